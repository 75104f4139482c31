// Stand-alone host program (tests/test_layout_cpu.py builds it with -fsanitize=address,undefined): the workspace layouts of
// csrc/hk_layout.h -- in-painting and block statistics -- hold what their kernels index, in the stated order, at the stated
// alignments, inside the stated total, and inside what the library reserved before the layouts were one function.
// What a piece has to hold is stated HERE from the kernels' index expressions (hk_inpaint.hip, hk_norm.hip), not taken from the
// layout functions.  Prints one line per family and returns 0, or the failed checks and 1.
#include <stdio.h>

#include "hk_layout.h"

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            ++failures;                                      \
            fprintf(stderr, "FAILED %s: ", #cond);           \
            fprintf(stderr, __VA_ARGS__);                    \
            fprintf(stderr, "\n");                           \
        }                                                    \
    } while (0)

// the packed search's finish tables as hk_inpaint.hip declares them: squared distances below (FAST_LAST + 1)^2 = 25^2
struct FastTablesMirror {
    double w[625];
    unsigned char root[625 + 7];
};

struct Piece {
    const char* name;
    size_t off, need, align;
};

static void inpaint_shape(int height, long long stride) {
    const hk::InpaintLayout l = hk::inpaint_layout(height, stride);
    const size_t px = (size_t)height * (size_t)stride;                           // entries [y * stride + x], y < height, x < stride
    const size_t words = (size_t)((height + 63) / 64) * (size_t)stride * 8;      // words [(y / 64) * stride + x] of 8 bytes
    const Piece pieces[] = {
        {"table", l.table, px * 4, 16},                                           // inpaint_table_kernel: 4-byte entries
        {"flag", l.flag, px, 16},                                                 // inpaint_flag_kernel / the fit kernel: bytes
        {"tie", l.tie, (size_t)(hk::TIE_N + 31) / 32 * 4, 256},                   // tie_kernel: TIE_N bits, stored as whole 32-bit words
        {"wtab", l.wtab, (size_t)hk::WTAB_N * 8, 256},                            // tie_kernel: WTAB_N doubles
        {"bits", l.bits, words, 256},                                             // inpaint_bits_kernel
        {"tbits", l.tbits, words, 256},                                           // inpaint_bits_kernel
        {"sbits", l.sbits, words, 256},                                           // inpaint_fill_fast_kernel
        {"ftab", l.ftab, sizeof(FastTablesMirror), 256},                          // fast_table_kernel
    };
    const int n = (int)(sizeof(pieces) / sizeof(pieces[0]));
    CHECK(l.table == 0, "%d x %lld: the table at %zu", height, stride, l.table);
    for (int i = 0; i < n; ++i) {
        const Piece& p = pieces[i];
        CHECK(p.off % p.align == 0, "%d x %lld: %s at %zu, not a multiple of %zu", height, stride, p.name, p.off, p.align);
        if (i + 1 < n)  // in the stated order, none reaching into the next
            CHECK(p.off + p.need <= pieces[i + 1].off, "%d x %lld: %s [%zu, +%zu) reaches %s at %zu", height, stride, p.name, p.off,
                  p.need, pieces[i + 1].name, pieces[i + 1].off);
        else
            CHECK(p.off + p.need <= l.total, "%d x %lld: %s [%zu, +%zu) past the total %zu", height, stride, p.name, p.off, p.need, l.total);
    }
    CHECK(hk::FAST_TABLES_BYTES == sizeof(FastTablesMirror), "FAST_TABLES_BYTES %zu", hk::FAST_TABLES_BYTES);
    // THE PARENT'S RESERVATION: inpaint_workspace_bytes() as it stood before inpaint_layout(), slack by hand
    const size_t parent = px * 5 + 1024 + hk::TIE_N / 8 + 256 + (size_t)hk::WTAB_N * 8 + 256 + 3 * (words + 256)
                          + sizeof(FastTablesMirror) + 256;
    CHECK(l.total <= parent, "%d x %lld: total %zu above the parent's %zu", height, stride, l.total, parent);
}

static void norm_shape(int n_bands, int height, int width) {
    const hk::NormLayout l = hk::norm_layout(n_bands, height, width);
    const size_t state = hk::NORM_WS_BYTES * (size_t)n_bands;                     // ws_all[band], band < n_bands
    const size_t cap = (size_t)((long long)height * width / 25 + 8192);           // values a compacted buffer may receive
    CHECK(state <= l.mid, "%d x %d x %d: the bands' state [0, +%zu) reaches the buffers at %zu", n_bands, height, width, state, l.mid);
    CHECK(l.mid % 256 == 0 && (l.cap_al * 4) % 256 == 0, "%d x %d x %d: buffers at %zu, %zu floats each", n_bands, height, width, l.mid, l.cap_al);
    CHECK(l.cap_al >= cap, "%d x %d x %d: %zu floats per buffer, %zu needed", n_bands, height, width, l.cap_al, cap);
    // mid_all[(band * 2 + q) * cap_al + i], q < 2, i < cap_al
    CHECK(l.mid + (size_t)n_bands * 2 * l.cap_al * 4 <= l.total, "%d x %d x %d: the buffers end past the total %zu", n_bands, height, width, l.total);
    // THE PARENT'S EXPRESSIONS (norm_workspace_bytes, launch_block_norm, launch_block_norm_split): the offsets are theirs
    const size_t p_mid = (state + 255) / 256 * 256, p_cap_al = (cap * 4 + 255) / 256 * 256 / 4;
    const size_t p_total = p_mid + (size_t)n_bands * 2 * ((cap * 4 + 255) / 256 * 256);
    CHECK(l.mid == p_mid && l.cap_al == p_cap_al && l.total == p_total, "%d x %d x %d: (%zu, %zu, %zu), the parent's (%zu, %zu, %zu)", n_bands,
          height, width, l.mid, l.cap_al, l.total, p_mid, p_cap_al, p_total);
}

int main() {
    const int heights[] = {1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 4097};
    const long long strides[] = {4, 8, 12, 260, 300, 16384, 1ll << 23};
    int n = 0;
    for (int h : heights)
        for (long long s : strides) inpaint_shape(h, s), ++n;
    printf("inpaint_layout: %d shapes\n", n);
    const int norm_shapes[][3] = {{1, 1, 1}, {1, 300, 70}, {3, 96, 300}, {4, 4096, 4096}};
    n = 0;
    for (const auto& s : norm_shapes) norm_shape(s[0], s[1], s[2]), ++n;
    printf("norm_layout: %d shapes\n", n);
    return failures ? 1 : 0;
}
