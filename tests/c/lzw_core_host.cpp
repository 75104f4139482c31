// The decoder core of hk_lzw.hip (homonim_amd/csrc/hk_lzw_core.h) as a plain C++ program: HKI_HOST, a loop over the lane index in
// place of the wave.  tests/test_lzw_cpu.py runs it over the stream set of tests/_lzw_streams.py, good and malformed.
//
//   lzw_core_host IN OUT
// IN:  uint32 n, then n times { uint32 size, uint32 raw, `size` stream bytes }   (little-endian)
// OUT: n times { uint32 status, `raw` bytes of the slot }
// Every stream is copied into a buffer that ends with it and every slot is exactly raw rounded up to 16 bytes, each from malloc, so
// that a build with a sanitizer sees any access outside them.
#define HKI_HOST
#include "hk_lzw_core.h"

#include <cstdio>
#include <cstdlib>

static bool read_u32(FILE* f, unsigned& v) {
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    v = b[0] | (b[1] << 8) | (b[2] << 16) | ((unsigned)b[3] << 24);
    return true;
}
static void write_u32(FILE* f, unsigned v) {
    const unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
    fwrite(b, 1, 4, f);
}

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
    unsigned n = 0;
    if (!read_u32(in, n)) return 2;
    hk::lzw::Shared* S = new hk::lzw::Shared();
    for (unsigned i = 0; i < n; ++i) {
        unsigned size = 0, raw = 0;
        if (!read_u32(in, size) || !read_u32(in, raw)) return fprintf(stderr, "stream %u: short file\n", i), 2;
        // (four streams of five start 1..4 bytes into their allocation: the 16-byte groups do not start at the stream's first
        // byte then; the allocation always ends with the stream)
        const unsigned shift = i % 5;
        unsigned char* buf = static_cast<unsigned char*>(malloc((size_t)size + shift + (size + shift ? 0 : 1)));
        unsigned char* stream = buf + shift;
        for (unsigned k = 0; k < shift; ++k) buf[k] = 0xA5;
        if (size && fread(stream, 1, size, in) != size) return fprintf(stderr, "stream %u: short file\n", i), 2;
        const size_t slot_bytes = ((size_t)raw + 15) / 16 * 16;
        unsigned char* slot = static_cast<unsigned char*>(calloc(slot_bytes ? slot_bytes : 16, 1));
        const unsigned status = hk::lzw::lzw_stream(*S, stream, size, slot, raw);
        write_u32(out, status);
        fwrite(slot, 1, raw, out);
        free(slot), free(buf);
    }
    delete S;
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
