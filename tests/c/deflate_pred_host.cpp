// The chunk coder of hk_deflate.hip (homonim_amd/csrc/hk_deflate_core.h) with the predictor mapping in front of it as a plain C++
// program: HKD_HOST, a loop over the thread index in place of the workgroup, the phases in the kernel's order, and the streams
// put together as deflate_gather_kernel does.  tests/test_out_profile_cpu.py builds it with -fsanitize=address,undefined and
// holds its streams to zlib and to the numpy statement of the predictors.
//
//   deflate_pred_host IN OUT
// IN:  uint32 n, then n times { uint32 sample bytes, uint32 tile, uint32 predictor, tile x tile x sample bytes of the raw tile }
// OUT: n times { uint32 size, `size` bytes: the tile's zlib stream }                                   (all little-endian)
// As in deflate_pred_chunk_kernel the WHOLE raw rows that a chunk and its history touch are staged, here into an allocation of
// exactly their size, and every byte of the chunk is predicted_byte() of its row: a read outside the row's allocation is the
// sanitizer's to find.  What lies in front of the tile's first byte is filled with a pattern no phase may read.
#define HKD_HOST
#include "hk_deflate_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace hk::deflate;

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

template <typename F>
static void all_threads(F f) {
    for (int tid = 0; tid < THREADS; ++tid) f(tid);
}

// one chunk: its block(s) appended to `stream`; -> (sum of bytes mod 65521) | (weighted sum mod 65521) << 16
static unsigned code_chunk(Shared& S, const unsigned char* tile_raw, int es, int tile, int predictor, int start, int n,
                           std::vector<unsigned char>& stream) {
    const int row_bytes = tile * es;
    const Chunk c = make_chunk(start, n, predictor_distance(predictor, es), row_bytes);
    const int hist = start < HIST ? start : HIST, first = start - hist;
    const int r_lo = first / row_bytes, r_hi = (start + n - 1) / row_bytes;
    const size_t staged = (size_t)(r_hi - r_lo + 1) * row_bytes;
    if (staged > sizeof(S.x)) {
        fprintf(stderr, "%zu staged bytes do not fit\n", staged);
        exit(3);
    }
    unsigned char* raw = static_cast<unsigned char*>(malloc(staged));
    memcpy(raw, tile_raw + (size_t)r_lo * row_bytes, staged);
    memset(S.data, 0xA5, sizeof(S.data));
    for (int q = first; q < start + n; ++q) {
        const int r = q / row_bytes, j = q - r * row_bytes;
        S.data[HIST + q - start] = (unsigned char)predicted_byte(raw + (size_t)(r - r_lo) * row_bytes, j, es, tile, predictor);
    }
    free(raw);
    all_threads([&](int t) { phase_scan(S, c, t); });
    for (int r = 0; r < 8; ++r) all_threads([&](int t) { phase_scan_round(S, t, r); });
    all_threads([&](int t) { phase_parse<false>(S, c, t); });
    all_threads([&](int t) { phase_walk(S, c, t); });
    all_threads([&](int t) { phase_parse<true>(S, c, t); });
    all_threads([&](int t) { phase_count(S, c, t); });
    all_threads([&](int t) { phase_sort_ll(S, t); });
    all_threads([&](int t) { phase_lengths(S, c, t); });
    all_threads([&](int t) { phase_codes(S, c, t); });
    all_threads([&](int t) { phase_sort_cl(S, t); });
    all_threads([&](int t) { phase_decide(S, c, t); });
    const unsigned dyn = S.sc[SC_DYN];
    if (dyn) {
        all_threads([&](int t) { phase_bits(S, c, t); });
        for (int r = 0; r < 8; ++r) all_threads([&](int t) { phase_bits_round(S, t, r); });
        all_threads([&](int t) { phase_emit(S, c, t); });
        for (unsigned k = 0; k < dyn; ++k) stream.push_back((unsigned char)(S.out[k >> 2] >> (8 * (k & 3))));
    } else {
        for (int k = 0; k < n + 5; ++k) stream.push_back((unsigned char)stored_byte(S, c, k));
    }
    return (S.sc[SC_AD_A] % 65521u) | ((S.sc[SC_AD_B] % 65521u) << 16);
}

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
    unsigned n_tiles = 0;
    if (!read_u32(in, n_tiles)) return 2;
    Shared* S = new Shared;
    for (unsigned i = 0; i < n_tiles; ++i) {
        unsigned es = 0, tile = 0, predictor = 0;
        if (!read_u32(in, es) || !read_u32(in, tile) || !read_u32(in, predictor)) return fprintf(stderr, "tile %u: short file\n", i), 2;
        if ((es != 1 && es != 2 && es != 4 && es != 8) || tile < 16 || tile > 512 || tile % 16 || predictor < 1 || predictor > 3)
            return fprintf(stderr, "tile %u: sample bytes %u, tile %u, predictor %u\n", i, es, tile, predictor), 2;
        const int tile_bytes = (int)(tile * tile * es);
        unsigned char* raw = static_cast<unsigned char*>(malloc(tile_bytes));
        if (fread(raw, 1, tile_bytes, in) != (size_t)tile_bytes) return fprintf(stderr, "tile %u: short file\n", i), 2;
        std::vector<unsigned char> stream = {0x78, 0x9C};
        unsigned s1 = 1, s2 = 0;
        for (int start = 0; start < tile_bytes; start += CHUNK) {
            const int n = tile_bytes - start < CHUNK ? tile_bytes - start : CHUNK;
            const unsigned v = code_chunk(*S, raw, (int)es, (int)tile, (int)predictor, start, n, stream);
            s2 = (s2 + (unsigned)n * s1 + (v >> 16)) % 65521u;
            s1 = (s1 + (v & 0xFFFFu)) % 65521u;
        }
        const unsigned char tail[6] = {0x03, 0x00, (unsigned char)(s2 >> 8), (unsigned char)s2, (unsigned char)(s1 >> 8), (unsigned char)s1};
        stream.insert(stream.end(), tail, tail + 6);
        write_u32(out, (unsigned)stream.size());
        fwrite(stream.data(), 1, stream.size(), out);
        free(raw);
    }
    delete S;
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
