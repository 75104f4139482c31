// hk_inflate_core.h -- the zlib (DEFLATE) decoder of hk_inflate.hip as functions over ONE WAVE's shared state: one wave of 64
// lanes inflates one stream (a tile or a strip of a GeoTIFF).  A host program compiles the same functions as plain C++ (HKI_HOST:
// no HIP; a loop over the lane index stands in for the wave, HKI_FOR_LANES), which is how every decision of the decoder is held to
// zlib without a GPU (tests/c/inflate_core_host.cpp).
//
// WHAT IS UNIFORM.  The bit buffer, the read and write positions, the status and every decoded symbol are the same in all lanes
// (`uni()` = readfirstlane: they live in scalar registers); the lanes only differ where bytes are moved: loading the input window,
// building the tables over the symbols, copying a match, flushing the ring.  Between a lane-parallel write of shared state and a
// read of it by other lanes stands HKI_SYNC (the workgroup IS the wave: a fence for the compiler, no waiting).
//
// INPUT.  The stream's bytes are read in aligned 16-byte groups, 64 at a time, into a window in LDS; a group that is not wholly
// inside [in, in + size) is read byte by byte and what lies outside reads as zero, so nothing outside the stream is ever loaded and
// bits past its end are zero bits.  `used` counts the bits consumed; a field that takes a bit past 8 * size sets TRUNCATED before
// its value is looked at.
//
// OUTPUT.  Bytes go into a ring of RING = 64 KiB in LDS: the last 32 KiB are the history matches read (only from here: global
// memory the kernel has written is never loaded), the part not yet flushed is at most FLUSH_AT + 258 + 15 bytes.  A match is
// copied by all lanes: output byte k takes the byte `dist` back for k < dist and byte k mod dist of those otherwise, so every read
// is of a byte that was there before the match began: the reads of a step cannot see its writes.  The ring leaves for the block's
// slot in 16-byte stores (the slot is raw size rounded up to 16); the Adler-32 is accumulated over what is flushed.
//
// STATUS.  The first error ends the block with its code (enum Status; HK_INFLATE_* of include/homonim_hk.h); nothing is written
// past the block's raw size (OVERRUN is found before the write), nothing is read before the first byte produced (FAR).
//
// TERMINATION.  The decoder is a loop of STEPS: a header field, a code length, a literal, a match, the end of a block, a round of
// a stored block's copy, the trailer.  Every step either takes at least one bit of input (every code of every table is at least
// one bit long; a stored block's header is at least 32 bits; a copy round of a non-empty stored block at least 8) or ends the
// block.  `used` never decreases, and a step that leaves used > 8 * size ends the block with TRUNCATED: at most 8 * size + 1
// steps.  The loops inside a step are bounded by constants: 15 code lengths, 258 bytes of a match, COPY_ROUND bytes of a stored
// block, 138 repeated lengths, FLUSH_AT + 273 bytes of a flush, 320 symbols of a table.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef HKI_HOST
#define HKI_FN inline
#define HKI_FOR_LANES for (int lane = 0; lane < ::hk::inflate::WAVE; ++lane)
#define HKI_SYNC() ((void)0)
#define HKI_UNROLL
namespace hk { namespace inflate {
typedef const unsigned char* in_ptr;      // the stream
typedef unsigned char* out_ptr;           // the block's slot
inline unsigned uni(unsigned v) { return v; }
inline void lds_add(unsigned* p, unsigned v) { *p += v; }
inline unsigned bitrev(unsigned v) {
    unsigned r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}
struct Quad { unsigned w[4]; };
inline Quad load_quad(in_ptr p) { Quad q; memcpy(&q, p, 16); return q; }
inline void store_quad(out_ptr p, const Quad& q) { memcpy(p, &q, 16); }
} }
#else
#include <hip/hip_runtime.h>
#define HKI_FN __device__ __forceinline__
#define HKI_FOR_LANES for (int lane = (int)threadIdx.x, once_ = 0; once_ < 1; ++once_)
#define HKI_SYNC() __syncthreads()
#define HKI_UNROLL _Pragma("unroll")
namespace hk { namespace inflate {
typedef const __attribute__((address_space(1))) unsigned char* in_ptr;
typedef __attribute__((address_space(1))) unsigned char* out_ptr;
__device__ __forceinline__ unsigned uni(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ void lds_add(unsigned* p, unsigned v) { atomicAdd(p, v); }   // (integer: any order, one result)
__device__ __forceinline__ unsigned bitrev(unsigned v) { return __brev(v); }
typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
struct Quad { unsigned w[4]; };   // (indexed by constants only)
__device__ __forceinline__ Quad load_quad(in_ptr p) {
    const u32x4_ v = *(const __attribute__((address_space(1))) u32x4_*)p;
    return Quad{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void store_quad(out_ptr p, const Quad& q) {
    *(__attribute__((address_space(1))) u32x4_*)p = u32x4_{q.w[0], q.w[1], q.w[2], q.w[3]};
}
} }
#endif

namespace hk {
namespace inflate {

constexpr int WAVE = 64;
constexpr unsigned RING = 65536, RING_MASK = RING - 1;   // the output ring (a power of two >= 64 KiB)
constexpr unsigned FLUSH_AT = 16384;                      // unflushed bytes at which the ring is flushed
constexpr unsigned COPY_ROUND = 4096;                     // bytes of a stored block copied per step
constexpr int WIN_WORDS = 4 * WAVE;                       // the input window: one 16-byte group per lane
constexpr int FAST_BITS = 10, FAST_SIZE = 1 << FAST_BITS; // codes up to this length are found by one table look-up
constexpr int CL_BITS = 7;                                // the code-length code: at most 7 bits
constexpr int NLL = 288, ND = 32, NCL = 19, MAXLENS = NLL + ND;
constexpr long long MAX_STREAM = 1ll << 28;               // bytes of a stream that are looked at (bit counts stay below 2^31)

// (HK_INFLATE_* of include/homonim_hk.h)
enum Status {
    OK = 0, TRUNCATED = 1, BAD_HEADER = 2, BAD_BLOCK = 3, BAD_STORED = 4, BAD_CODE = 5, BAD_SYMBOL = 6, FAR = 7, OVERRUN = 8,
    SHORT = 9, ADLER = 10
};

// one prefix code: the look-up table of its short codes and the canonical description of the long ones
struct Code {
    unsigned short count[16];    // codes per length
    unsigned short first[16];    // first canonical code of a length
    unsigned short offset[16];   // index in `sorted` of the first symbol of a length
};

struct Shared {
    alignas(16) unsigned char ring[RING];
    alignas(16) unsigned in[WIN_WORDS];
    alignas(16) unsigned short fast_ll[FAST_SIZE];   // (symbol << 4) | length, 0: no code of at most FAST_BITS bits starts so
    alignas(16) unsigned short fast_d[FAST_SIZE];    // (the code-length code is built here too: it is gone when the others are made)
    unsigned short sorted_ll[NLL], sorted_d[ND];     // symbols by (length, symbol)
    alignas(4) unsigned char lens[MAXLENS];          // code lengths: literal/length symbols, then the distance symbols
    alignas(4) unsigned char cl_lens[NCL + 1];
    Code ll, d;
    unsigned cnt[16];                                // codes per length while a table is built
    unsigned ad[2];                                  // a flush's Adler sums
};

// what the wave carries in scalar registers
struct State {
    in_ptr in;              // the stream, and its first byte's place in its 16-byte group
    unsigned skew;
    unsigned size;          // its bytes (at most MAX_STREAM)
    out_ptr slot;           // the block's bytes in global memory
    unsigned raw;           // how many there have to be
    unsigned long long bb;  // the bit buffer: the next `nbits` bits of the stream, the first one lowest
    unsigned nbits;
    unsigned wpos;          // the next word to enter the bit buffer (a word index from the stream's aligned-down start)
    unsigned win0;          // first word of the window in LDS (a multiple of 4); 0xFFFFFFFF: none loaded
    unsigned used, limit;   // bits consumed; 8 * size
    unsigned out, flushed;  // bytes produced / of them in the slot
    unsigned s1, s2;        // Adler-32 of the flushed bytes
    unsigned status;
};

// the order in which a dynamic header stores the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
HKI_FN int cl_order(int i) { return i < 3 ? 16 + i : (i == 3 ? 0 : ((i & 1) ? 7 - ((i - 5) >> 1) : 8 + ((i - 4) >> 1))); }
// length symbol 257..285 -> (base, extra bits); distance symbol 0..29 -> (base, extra bits): arithmetic, no tables
HKI_FN void length_base(unsigned sym, unsigned& base, unsigned& extra) {
    const unsigned c = sym - 257;
    if (c < 8) base = 3 + c, extra = 0;
    else if (c == 28) base = 258, extra = 0;
    else extra = (c >> 2) - 1, base = 3 + ((4 + (c & 3)) << extra);
}
HKI_FN void dist_base(unsigned sym, unsigned& base, unsigned& extra) {
    if (sym < 4) base = 1 + sym, extra = 0;
    else extra = (sym >> 1) - 1, base = 1 + ((2 + (sym & 1)) << extra);
}

HKI_FN void fail(State& s, unsigned code) {
    if (!s.status) s.status = code;
}

// ---- input ----------------------------------------------------------------------------------------------------------------
// the 64 groups from word `w0` (a multiple of 4) on into LDS
HKI_FN void load_window(Shared& S, State& s, unsigned w0) {
    HKI_SYNC();   // (the window's last readers are done)
    HKI_FOR_LANES {
        const long long gs = 4ll * w0 + 16ll * lane - (long long)s.skew;   // the group's first byte within the stream
        Quad q = {{0, 0, 0, 0}};
        if (gs >= 0 && gs + 16 <= (long long)s.size) {
            q = load_quad(s.in + gs);
        } else if (gs > -16 && gs < (long long)s.size) {
HKI_UNROLL
            for (int j = 0; j < 16; ++j)
                if (gs + j >= 0 && gs + j < (long long)s.size) q.w[j >> 2] |= (unsigned)s.in[gs + j] << (8 * (j & 3));
        }
        S.in[4 * lane + 0] = q.w[0], S.in[4 * lane + 1] = q.w[1], S.in[4 * lane + 2] = q.w[2], S.in[4 * lane + 3] = q.w[3];
    }
    HKI_SYNC();
    s.win0 = w0;
}

HKI_FN unsigned next_word(Shared& S, State& s) {
    const unsigned w = s.wpos++;
    if (4ull * w >= (unsigned long long)s.skew + s.size) return 0;   // past the end: zero bits, no load
    if (s.win0 == 0xFFFFFFFFu || w - s.win0 >= (unsigned)WIN_WORDS) load_window(S, s, w & ~3u);
    return uni(S.in[w - s.win0]);
}

// at least 32 bits in the buffer
HKI_FN void refill(Shared& S, State& s) {
    if (s.nbits < 32) {
        s.bb |= (unsigned long long)next_word(S, s) << s.nbits;
        s.nbits += 32;
    }
}

// the bit buffer starts anew at byte `pos` of the stream
HKI_FN void seek(Shared& S, State& s, unsigned pos) {
    const unsigned at = s.skew + pos;
    s.wpos = at >> 2;
    s.bb = 0, s.nbits = 0, s.used = 8 * pos;
    refill(S, s);
    s.bb >>= 8 * (at & 3), s.nbits -= 8 * (at & 3);
    refill(S, s);
}

HKI_FN void drop(State& s, unsigned n) {   // n <= nbits
    s.bb >>= n, s.nbits -= n, s.used += n;
    if (s.used > s.limit) fail(s, TRUNCATED);
}
HKI_FN unsigned peek(const State& s, unsigned n) { return (unsigned)s.bb & ((1u << n) - 1); }
// n <= 16 bits (refill first: there are at least 32)
HKI_FN unsigned take(State& s, unsigned n) {
    const unsigned v = peek(s, n);
    drop(s, n);
    return v;
}

// ---- tables ---------------------------------------------------------------------------------------------------------------
// The code of `n` symbols with lengths `lens`: counts, the over-subscription and completeness rules of zlib (an incomplete set is
// accepted only as ONE code of length 1, and never for the code-length code; no code at all is an empty table, in which every
// look-up fails), first codes and offsets, then per symbol (lanes in parallel) its rank among the symbols of its length, which
// gives its canonical code: the look-up entries of a short code, its place in `sorted`.
HKI_FN void build_code(Shared& S, State& s, const unsigned char* lens, int n, Code& c, unsigned short* fast, int fast_bits,
                       unsigned short* sorted, bool is_cl) {
    HKI_SYNC();
    HKI_FOR_LANES {
        if (lane < 16) S.cnt[lane] = 0;
        // (2 << fast_bits bytes: 16 per lane and round)
        for (int k = lane; k < (2 << fast_bits) / 16; k += WAVE) {
            unsigned* const p = reinterpret_cast<unsigned*>(fast) + 4 * k;
            p[0] = 0, p[1] = 0, p[2] = 0, p[3] = 0;
        }
    }
    HKI_SYNC();
    HKI_FOR_LANES {
        for (int i = lane; i < n; i += WAVE)
            if (lens[i]) lds_add(&S.cnt[lens[i] & 15], 1);
    }
    HKI_SYNC();
    int left = 1, max_len = 0;
    unsigned code = 0, off = 0;
    bool over = false;
    for (int l = 1; l <= 15; ++l) {
        const unsigned k = uni(S.cnt[l]);
        left = 2 * left - (int)k;
        if (left < 0) over = true, left = 0;   // (and stays refused)
        if (k) max_len = l;
        code <<= 1;
        HKI_FOR_LANES {
            if (lane == 0) c.count[l] = (unsigned short)k, c.first[l] = (unsigned short)code, c.offset[l] = (unsigned short)off;
        }
        code += k, off += k;
    }
    if (over || (left > 0 && max_len != 0 && (is_cl || max_len != 1))) {
        fail(s, BAD_CODE);
        return;
    }
    HKI_SYNC();
    HKI_FOR_LANES {
        for (int i = lane; i < n; i += WAVE) {
            const unsigned l = lens[i] & 15;
            if (!l) continue;
            unsigned rank = 0;
            for (int o = 0; o < i; ++o) rank += lens[o] == l;
            sorted[c.offset[l] + rank] = (unsigned short)i;
            if ((int)l <= fast_bits) {
                const unsigned r = bitrev(c.first[l] + rank) >> (32 - l);
                for (unsigned e = r; e < (1u << fast_bits); e += 1u << l) fast[e] = (unsigned short)((i << 4) | l);
            }
        }
    }
    HKI_SYNC();
}

// The next symbol of a code.  -> the symbol, or 0xFFFF where the bits are no code of the set (status is set then, to `bad`).
HKI_FN unsigned decode(Shared& S, State& s, const Code& c, const unsigned short* fast, int fast_bits, const unsigned short* sorted,
                       unsigned bad) {
    (void)S;
    const unsigned e = uni(fast[peek(s, fast_bits)]);
    if (e) {
        drop(s, e & 15);
        return e >> 4;
    }
    // a longer code: the canonical walk over the lengths, on the bits in code order
    const unsigned rev = bitrev(peek(s, 15)) >> 17;
    for (int l = fast_bits + 1; l <= 15; ++l) {
        const unsigned k = (rev >> (15 - l)) - uni(c.first[l]);
        if (k < uni(c.count[l])) {
            drop(s, l);
            return uni(sorted[uni(c.offset[l]) + k]);
        }
    }
    drop(s, 1);      // (a step takes a bit)
    fail(s, bad);
    return 0xFFFFu;
}

// the two codes of a fixed block, from the constant lengths
HKI_FN void build_fixed(Shared& S, State& s) {
    HKI_SYNC();
    HKI_FOR_LANES {
        for (int i = lane; i < NLL; i += WAVE) S.lens[i] = (unsigned char)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        if (lane < ND) S.lens[NLL + lane] = 5;
    }
    build_code(S, s, S.lens, NLL, S.ll, S.fast_ll, FAST_BITS, S.sorted_ll, false);
    build_code(S, s, S.lens + NLL, ND, S.d, S.fast_d, FAST_BITS, S.sorted_d, false);
}

// the header of a dynamic block and its two codes
HKI_FN void build_dynamic(Shared& S, State& s) {
    refill(S, s);
    const unsigned hlit = take(s, 5) + 257, hdist = take(s, 5) + 1, hclen = take(s, 4) + 4;
    if (s.status) return;
    if (hlit > 286 || hdist > 30) return fail(s, BAD_CODE);
    HKI_SYNC();
    HKI_FOR_LANES {
        if (lane < NCL + 1) S.cl_lens[lane] = 0;
    }
    HKI_SYNC();
    for (unsigned i = 0; i < hclen; ++i) {
        refill(S, s);
        const unsigned v = take(s, 3);
        HKI_FOR_LANES {
            if (lane == 0) S.cl_lens[cl_order((int)i)] = (unsigned char)v;
        }
    }
    if (s.status) return;
    // (the code-length code borrows the distance code's tables)
    build_code(S, s, S.cl_lens, NCL, S.d, S.fast_d, CL_BITS, S.sorted_d, true);
    if (s.status) return;
    const unsigned total = hlit + hdist;
    unsigned i = 0, prev = 0;
    while (i < total) {
        refill(S, s);
        const unsigned sym = decode(S, s, S.d, S.fast_d, CL_BITS, S.sorted_d, BAD_CODE);
        if (s.status) return;
        unsigned rep = 1, v = sym;
        if (sym == 16) {
            if (i == 0) return fail(s, BAD_CODE);
            rep = 3 + take(s, 2), v = prev;
        } else if (sym == 17) {
            rep = 3 + take(s, 3), v = 0;
        } else if (sym == 18) {
            rep = 11 + take(s, 7), v = 0;
        }
        if (s.status) return;
        if (i + rep > total) return fail(s, BAD_CODE);
        HKI_FOR_LANES {
            for (unsigned k = (unsigned)lane; k < rep; k += WAVE) S.lens[i + k] = (unsigned char)v;
        }
        i += rep, prev = v;
    }
    HKI_SYNC();
    if (uni(S.lens[256]) == 0) return fail(s, BAD_CODE);   // no end-of-block code
    build_code(S, s, S.lens, (int)hlit, S.ll, S.fast_ll, FAST_BITS, S.sorted_ll, false);
    if (s.status) return;
    // (the distance lengths follow the literal/length ones; the tables of the code-length code are overwritten)
    build_code(S, s, S.lens + hlit, (int)hdist, S.d, S.fast_d, FAST_BITS, S.sorted_d, false);
}

// ---- output ---------------------------------------------------------------------------------------------------------------
// Bytes [flushed, upto) of the block from the ring to the slot, 16 per lane and store (`flushed` is a multiple of 16; a last group
// that is not whole is stored whole: the slot is the raw size rounded up to 16), and into the Adler-32.
HKI_FN void flush(Shared& S, State& s, unsigned upto) {
    const unsigned n = upto - s.flushed;
    if (n == 0) return;
    HKI_SYNC();
    HKI_FOR_LANES {
        if (lane < 2) S.ad[lane] = 0;
    }
    HKI_SYNC();
    HKI_FOR_LANES {
        unsigned a = 0, b = 0;
        for (unsigned g = 16u * lane; g < n; g += 16u * WAVE) {   // byte g of the flush
            const unsigned* const w = reinterpret_cast<const unsigned*>(&S.ring[(s.flushed + g) & RING_MASK]);
            const Quad q = {{w[0], w[1], w[2], w[3]}};
            store_quad(s.slot + s.flushed + g, q);
HKI_UNROLL
            for (int j = 0; j < 16; ++j) {
                const unsigned v = g + j < n ? (q.w[j >> 2] >> (8 * (j & 3))) & 255u : 0u;
                a += v, b += (n - g - j) * v;   // (n - g - j) * v < 2^15 * 2^8; 16 * 17 of them: below 2^32
            }
        }
        lds_add(&S.ad[0], a);               // at most 255 n
        lds_add(&S.ad[1], b % 65521u);      // 64 values below 65521
    }
    HKI_SYNC();
    // s1' = s1 + sum d; s2' = s2 + n s1 + sum (n - i) d_i   (n < 2^15, s1 < 2^16)
    s.s2 = (s.s2 + n * s.s1 + uni(S.ad[1])) % 65521u;
    s.s1 = (s.s1 + uni(S.ad[0])) % 65521u;
    s.flushed = upto;
}
HKI_FN void maybe_flush(Shared& S, State& s) {
    if (s.out - s.flushed >= FLUSH_AT) flush(S, s, s.out & ~15u);
}

// ---- the blocks -----------------------------------------------------------------------------------------------------------
HKI_FN void stored_block(Shared& S, State& s) {
    drop(s, (0u - s.used) & 7);   // to the byte boundary
    refill(S, s);
    const unsigned len = take(s, 16);
    refill(S, s);
    const unsigned nlen = take(s, 16);
    if (s.status) return;
    if ((len ^ nlen) != 0xFFFFu) return fail(s, BAD_STORED);
    unsigned pos = s.used >> 3;                       // the first data byte; pos <= size here
    if (len > s.size - pos) return fail(s, TRUNCATED);
    if (len > s.raw - s.out) return fail(s, OVERRUN);
    for (unsigned left = len; left > 0;) {
        const unsigned n = left < COPY_ROUND ? left : COPY_ROUND;
        HKI_FOR_LANES {
            for (unsigned k = (unsigned)lane; k < n; k += WAVE) S.ring[(s.out + k) & RING_MASK] = s.in[pos + k];
        }
        HKI_SYNC();
        s.out += n, pos += n, left -= n;
        maybe_flush(S, s);
    }
    seek(S, s, pos);
}

// the tokens of a fixed or dynamic block, up to its end-of-block symbol
HKI_FN void coded_block(Shared& S, State& s) {
    for (;;) {
        refill(S, s);
        const unsigned sym = decode(S, s, S.ll, S.fast_ll, FAST_BITS, S.sorted_ll, BAD_SYMBOL);
        if (s.status) return;
        if (sym < 256) {
            if (s.out >= s.raw) return fail(s, OVERRUN);
            HKI_FOR_LANES {
                if (lane == 0) S.ring[s.out & RING_MASK] = (unsigned char)sym;
            }
            HKI_SYNC();
            s.out += 1;
        } else if (sym == 256) {
            return;
        } else {
            if (sym >= 286) return fail(s, BAD_SYMBOL);
            unsigned len, dist, extra;
            length_base(sym, len, extra);
            len += take(s, extra);
            refill(S, s);
            const unsigned dsym = decode(S, s, S.d, S.fast_d, FAST_BITS, S.sorted_d, BAD_SYMBOL);
            if (s.status) return;
            if (dsym >= 30) return fail(s, BAD_SYMBOL);
            dist_base(dsym, dist, extra);
            dist += take(s, extra);
            if (s.status) return;
            if (dist > s.out) return fail(s, FAR);
            if (len > s.raw - s.out) return fail(s, OVERRUN);
            const unsigned from = s.out - dist;
            HKI_FOR_LANES {
                // (all reads are of bytes in front of s.out: none of this match's own)
                unsigned char v[5];   // (indexed by the unrolled counter only)
HKI_UNROLL
                for (int r = 0; r < 5; ++r) {
                    const unsigned k = (unsigned)lane + 64u * r;
                    if (k < len) v[r] = S.ring[(from + (dist < len ? k % dist : k)) & RING_MASK];
                }
HKI_UNROLL
                for (int r = 0; r < 5; ++r) {
                    const unsigned k = (unsigned)lane + 64u * r;
                    if (k < len) S.ring[(s.out + k) & RING_MASK] = v[r];
                }
            }
            HKI_SYNC();
            s.out += len;
        }
        maybe_flush(S, s);
    }
}

// One stream into its slot: -> the status.  `size` bytes at `in`; `raw` bytes are expected; the slot has raw rounded up to 16.
HKI_FN unsigned inflate_stream(Shared& S, in_ptr in, long long size, out_ptr slot, unsigned raw) {
    State s;
    s.in = in, s.skew = (unsigned)((uintptr_t)in & 15u);
    s.size = (unsigned)(size < 0 ? 0 : size > MAX_STREAM ? MAX_STREAM : size);
    s.slot = slot, s.raw = raw;
    s.limit = 8 * s.size, s.out = 0, s.flushed = 0, s.s1 = 1, s.s2 = 0, s.status = OK, s.win0 = 0xFFFFFFFFu;
    seek(S, s, 0);
    // the zlib header: method 8, window at most 32 KiB, the check bits, no preset dictionary
    const unsigned cmf = take(s, 8), flg = take(s, 8);
    if (s.status) return s.status;
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) return BAD_HEADER;
    for (unsigned last = 0; !last;) {
        refill(S, s);
        last = take(s, 1);
        const unsigned type = take(s, 2);
        if (s.status) return s.status;
        if (type == 3) return BAD_BLOCK;
        if (type == 0) {
            stored_block(S, s);
        } else {
            if (type == 1) build_fixed(S, s);
            else build_dynamic(S, s);
            if (s.status) return s.status;
            coded_block(S, s);
        }
        if (s.status) return s.status;
    }
    if (s.out != s.raw) return SHORT;
    flush(S, s, s.out);
    // the trailer: the Adler-32 of the raw bytes, big-endian, from the next byte boundary; what follows it is not looked at
    drop(s, (0u - s.used) & 7);
    unsigned adler = 0;
    for (int i = 0; i < 4; ++i) {
        refill(S, s);
        adler = (adler << 8) | take(s, 8);
    }
    if (s.status) return s.status;
    return adler == ((s.s2 << 16) | s.s1) ? (unsigned)OK : (unsigned)ADLER;
}

}  // namespace inflate
}  // namespace hk
