// hk_layout.h -- where the pieces of the device workspaces lie.  Plain C++ without HIP: the launchers (hk_inpaint.hip, hk_norm.hip), the
// host layer (hk_api.hip) and a stand-alone host program (tests/c/inpaint_layout_host.cpp) read the same statements.
#pragma once
#include <stddef.h>

namespace hk {

// Bump allocation inside one device buffer: every piece starts at a multiple of `align` bytes FROM THE BUFFER'S BASE and is padded
// to one, in the order it is taken.  (Nothing here looks at an address: where a piece lies does not depend on the base handed in.)
struct SlabLayout {
    size_t total = 0;
    size_t take(size_t bytes, size_t align = 256) {
        const size_t off = (total + align - 1) / align * align;
        total = (off + bytes + align - 1) / align * align;
        return off;
    }
};

// ---- In-painting (hk_inpaint.hip) --------------------------------------------------------------------------------------------------
constexpr int WORD_ROWS = 64;       // rows per word of the column bit planes
// (the search distance, FILL_MAX_DIST = 100, stays with the kernels: hk_inpaint.hip asserts the two sizes against it)
constexpr int TIE_N = 2 * 102 * 102;  // > the largest squared distance the search can meet (100^2 + 101^2): bits of the tie bitmap
constexpr int WTAB_N = 100 * 100 + 1;  // weights 1 / qd of the accepted distances (qd <= max_dist = 100)
constexpr size_t FAST_TABLES_BYTES = 5632;  // sizeof(FastTables), the packed search's finish tables (hk_inpaint.hip asserts it)

// Byte offsets of the workspace's pieces from its base, in this order.  The base must be 16-byte aligned (launch_inpaint_offsets
// checks it): the table is staged by 16-byte loads and stored as 8-byte pairs, rows being padded to quads (stride % 4 == 0).
struct InpaintLayout {
    size_t table;  // the distance table: height x stride words of 4 bytes, (down^2 << 16) | up^2; at 0
    size_t flag;   // the source flags: height x stride bytes; a multiple of 16 behind the table, every later piece at one of 256
    size_t tie;    // the tie bitmap: TIE_N bits as 32-bit words
    size_t wtab;   // the weight table: WTAB_N doubles
    size_t bits, tbits, sbits;  // column bit planes (sources, targets, targets the packed search left over): ceil(height / WORD_ROWS) x stride words of 8 bytes
    size_t ftab;   // the packed search's tables (FastTables)
    size_t total;
};
inline InpaintLayout inpaint_layout(int height, long long stride) {
    const size_t px = (size_t)height * (size_t)stride;
    const size_t plane_words = (size_t)((height + WORD_ROWS - 1) / WORD_ROWS) * (size_t)stride;
    SlabLayout s;
    InpaintLayout l;
    l.table = s.take(px * 4, 16), l.flag = s.take(px, 16);
    l.tie = s.take((size_t)(TIE_N + 31) / 32 * 4), l.wtab = s.take((size_t)WTAB_N * 8);
    l.bits = s.take(plane_words * 8), l.tbits = s.take(plane_words * 8), l.sbits = s.take(plane_words * 8);
    l.ftab = s.take(FAST_TABLES_BYTES);
    l.total = s.total;
    return l;
}

// ---- Block statistics (hk_norm.hip): [n_bands x NormWS | n_bands x [src | ref] compacted buffers], height x width = the (largest) plane
constexpr size_t NORM_WS_BYTES = 196824;  // sizeof(NormWS), the per-band state (hk_norm.hip asserts it)
inline size_t norm_mid_capacity(long long n_px) { return (size_t)(n_px / 25 + 8192); }  // values per buffer: 4 % of the block + slack
struct NormLayout {
    size_t mid;     // byte offset of the compacted buffers
    size_t cap_al;  // floats per compacted buffer (a multiple of 64: every buffer starts 256-byte aligned)
    size_t total;
};
inline NormLayout norm_layout(int n_bands, int height, int width) {
    SlabLayout s, one;
    NormLayout l;
    s.take(NORM_WS_BYTES * (size_t)n_bands);
    one.take(norm_mid_capacity((long long)height * width) * sizeof(float));  // a buffer, padded
    l.cap_al = one.total / sizeof(float);
    l.mid = s.take((size_t)n_bands * 2 * one.total);
    l.total = s.total;
    return l;
}

}  // namespace hk
