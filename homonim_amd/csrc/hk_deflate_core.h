// hk_deflate_core.h -- the per-chunk DEFLATE encoder of hk_deflate.hip as a sequence of PHASES over one workgroup's shared
// state.  A phase is a function of (shared state, chunk, thread index) that reads only what earlier phases wrote; the kernel
// runs phase after phase with a barrier between two, and a host program can run the same phases with a loop over the thread
// index in place of the workgroup (HKD_HOST: plain C++, no HIP), which is how the bit stream is tested against zlib without a GPU.
// Nothing in here touches global memory.  The stream format is stated at the top of hk_deflate.hip.  predicted_byte() is the TIFF
// predictors as a byte mapping, for the kernel's staging and the host program alike (tests/c/deflate_pred_host.cpp).
#pragma once
#include <stdint.h>

#ifdef HKD_HOST
#define HKD_FN inline
namespace hk { namespace deflate {
inline void lds_add(unsigned* p, unsigned v) { *p += v; }
inline void lds_or(unsigned* p, unsigned v) { *p |= v; }
inline int msb(unsigned v) { return 31 - __builtin_clz(v); }
inline unsigned bitrev(unsigned v) {
    unsigned r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}
} }
#else
#include <hip/hip_runtime.h>
#define HKD_FN __device__ __forceinline__
namespace hk { namespace deflate {
// (integer atomics on LDS: the result does not depend on the order the lanes arrive in)
__device__ __forceinline__ void lds_add(unsigned* p, unsigned v) { atomicAdd(p, v); }
__device__ __forceinline__ void lds_or(unsigned* p, unsigned v) { atomicOr(p, v); }
__device__ __forceinline__ int msb(unsigned v) { return 31 - __clz((int)v); }
__device__ __forceinline__ unsigned bitrev(unsigned v) { return __brev(v); }
} }
#endif

namespace hk {
namespace deflate {

constexpr int CHUNK = 16384;          // HK_DEFLATE_CHUNK: raw bytes per block
constexpr int HIST = 4096;            // history kept in front of a chunk: the largest candidate distance (512 samples of 8 bytes)
constexpr int THREADS = 256;
constexpr int SEG = CHUNK / THREADS;  // consecutive positions owned by one thread
constexpr int SLOT = (CHUNK + 5 + 15) / 16 * 16;   // output slot of a chunk: its stored form, rounded up to 16
constexpr int NLL = 286, ND = 30, NCL = 19, MAXHDR = NLL + ND, MAXDEPTH = 40;
constexpr unsigned NONE = 0xFFFFu;

enum { SC_NUSED, SC_NRLE, SC_HLIT, SC_HDIST, SC_HCLEN, SC_BODY, SC_HDR, SC_DYN, SC_AD_A, SC_AD_B, SC_N };

struct Shared {
    alignas(16) unsigned char data[HIST + CHUNK];   // [HIST + p] = byte p of the chunk; the bytes in front of it are the tile's
    unsigned short x[CHUNK];                        // phase 3: where the token chain leaves the segment; from phase 5: the token
    alignas(16) unsigned out[SLOT / 4 + 4];         // the block's bits
    unsigned hll[NLL], hd[ND], hcl[NCL];            // symbol counts
    unsigned key[NLL];                              // counts in ascending order, then the scratch of the code construction
    unsigned short sym[NLL];                        // the symbols in that order
    unsigned numc[MAXDEPTH + 1];                    // codes per length
    unsigned first[16];                             // first canonical code per length
    unsigned char lll[NLL], dl[ND], cll[NCL];       // code lengths
    unsigned short llc[NLL], dc[ND], clc[NCL];      // codes, bit-reversed: ready to be put LSB first
    unsigned char rsym[MAXHDR], rext[MAXHDR];       // the code-length header: symbols 0..18 and the value of their extra bits
    unsigned short fz[2][2][THREADS];               // per candidate: first position of a segment at which the run breaks (scanned)
    unsigned cnt[2][THREADS];                       // bits per segment (scanned)
    unsigned short entry[THREADS];                  // first token start inside the segment, or NONE
    unsigned sc[SC_N];
};

struct Chunk {
    int n;          // raw bytes of this chunk (a multiple of 256)
    int start;      // its first byte within the tile
    // the two candidate distances (0: sample size, 1: row length in bytes), their distance symbol, number of extra bits and extra
    // value: scalars picked by a select, not arrays -- an array indexed by a lane's token would live in scratch memory
    int d0, d1, dcode0, dcode1, dext0, dext1, dextv0, dextv1;
    HKD_FN int d(int k) const { return k ? d1 : d0; }
    HKD_FN int dcode(int k) const { return k ? dcode1 : dcode0; }
    HKD_FN int dext(int k) const { return k ? dext1 : dext0; }
    HKD_FN int dextv(int k) const { return k ? dextv1 : dextv0; }
};

HKD_FN void distance_code(int d, int& code, int& ext, int& extv) {
    const unsigned m = (unsigned)d - 1;
    if (m < 4) {
        code = (int)m, ext = 0, extv = 0;
    } else {
        const int e = msb(m) - 1;
        code = (e << 1) + (int)(m >> e), ext = e, extv = (int)(m & ((1u << e) - 1));
    }
}

HKD_FN Chunk make_chunk(int start, int n, int sample_bytes, int row_bytes) {
    Chunk c;
    c.n = n, c.start = start, c.d0 = sample_bytes, c.d1 = row_bytes;
    distance_code(c.d0, c.dcode0, c.dext0, c.dextv0);
    distance_code(c.d1, c.dcode1, c.dext1, c.dextv1);
    return c;
}

// ---- the TIFF predictors (tag 317) as a byte mapping: predicted byte j of ONE tile row from that row's raw bytes -- `tile`
// little-endian samples of `es` bytes, B = tile x es bytes.  The coder compresses the predicted bytes; the kernel's staging
// (deflate_pred_chunk_kernel) and the host build call this one function.
//   1: the byte itself.
//   2 (integers): p[i] = s[i] - s[i - 1] modulo 2^(8 es), p[0] = s[0]; samples stay little-endian.  Byte b of a difference needs
//      bytes 0..b of both samples: the borrow runs upwards.
//   3 (floats; libtiff's floating-point predictor): the row regrouped into `es` planes of `tile` bytes, most significant byte
//      first -- q[p tile + i] = byte es - 1 - p of sample i -- then d[0] = q[0], d[j] = q[j] - q[j - 1] modulo 256 over all B
//      bytes, across the plane boundaries.
// predictor_distance: the first candidate distance of the parse that goes with a predictor (the second is always the row length);
// under predictor 3 the bytes of a plane repeat at distance 1, not at the sample size.
HKD_FN int predictor_distance(int predictor, int es) { return predictor == 3 ? 1 : es; }

HKD_FN unsigned predicted_byte(const unsigned char* row, int j, int es, int tile, int predictor) {
    if (predictor == 2) {
        const int b = j & (es - 1), at = j - b;   // (es is a power of two)
        int borrow = 0, v = 0;
        for (int k = 0; k <= b; ++k) {
            v = (int)row[at + k] - (at ? (int)row[at - es + k] : 0) - borrow;
            borrow = v < 0;
        }
        return (unsigned)v & 0xFFu;
    }
    if (predictor == 3) {
        const int p = j / tile, i = j - p * tile, at = es - 1 - p;
        const unsigned cur = row[i * es + at];
        const unsigned prev = j == 0 ? 0u : (i ? row[(i - 1) * es + at] : row[(tile - 1) * es + at + 1]);
        return (cur - prev) & 0xFFu;
    }
    return row[j];
}

// length 3..258 -> (symbol - 257, number of extra bits, their value)
HKD_FN void length_code(int len, int& code, int& ext, int& extv) {
    const unsigned l = (unsigned)len - 3;
    if (l < 8) code = (int)l, ext = 0, extv = 0;
    else if (len == 258) code = 28, ext = 0, extv = 0;
    else {
        const int e = msb(l) - 2;
        code = (e << 2) + (int)(l >> e), ext = e, extv = (int)(l & ((1u << e) - 1));
    }
}
HKD_FN int ll_extra_bits(int s) { return (s < 265 || s == 285) ? 0 : (s - 261) >> 2; }

HKD_FN bool eq(const Shared& S, const Chunk& c, int k, int p) {
    return (c.start + p >= c.d(k)) && S.data[HIST + p] == S.data[HIST + p - c.d(k)];
}

HKD_FN void put_bits(Shared& S, unsigned pos, unsigned v, int nbits) {
    if (nbits == 0) return;
    const unsigned w = pos >> 5, sh = pos & 31;
    lds_or(&S.out[w], v << sh);
    if (sh + (unsigned)nbits > 32) lds_or(&S.out[w + 1], v >> (32 - sh));
}

// ---- phase 1: clear the tables; per segment and candidate the first position at which byte[p] != byte[p - d]; Adler sums
HKD_FN void phase_scan(Shared& S, const Chunk& c, int tid) {
    for (int i = tid; i < NLL; i += THREADS) S.hll[i] = 0, S.lll[i] = 0, S.llc[i] = 0;
    if (tid < ND) S.hd[tid] = 0, S.dl[tid] = 0, S.dc[tid] = 0;
    if (tid < SC_N) S.sc[tid] = 0;
    for (int i = tid; i < SLOT / 4 + 4; i += THREADS) S.out[i] = 0;
    const int p0 = tid * SEG;
    unsigned f0 = NONE, f1 = NONE, a = 0, b = 0;
    for (int j = SEG - 1; j >= 0; --j) {
        const int p = p0 + j;
        if (p >= c.n) {
            f0 = f1 = (unsigned)p;
            continue;
        }
        if (!eq(S, c, 0, p)) f0 = (unsigned)p;
        if (!eq(S, c, 1, p)) f1 = (unsigned)p;
        const unsigned v = S.data[HIST + p];
        a += v, b += (unsigned)(c.n - p) * v;   // at most 64 x 16384 x 255 < 2^32
    }
    S.fz[0][0][tid] = (unsigned short)f0, S.fz[0][1][tid] = (unsigned short)f1;
    S.entry[tid] = (unsigned short)NONE;
    S.cnt[0][tid] = 0;
    S.cnt[1][tid] = a;            // (parked until the tables are cleared: summed in the first scan round)
    S.x[p0] = (unsigned short)(b % 65521u);   // (parked likewise; x is written from phase 3 on)
}

// ---- phase 2, rounds 0..7: suffix minimum of fz over the segments (fz[0] -> fz[1] -> fz[0] ...; the result is in fz[0])
HKD_FN void phase_scan_round(Shared& S, int tid, int r) {
    const int from = r & 1, to = from ^ 1, o = tid + (1 << r);
    for (int k = 0; k < 2; ++k) {
        const unsigned here = S.fz[from][k][tid], there = o < THREADS ? S.fz[from][k][o] : NONE;
        S.fz[to][k][tid] = (unsigned short)(here < there ? here : there);
    }
    if (r == 0) {
        lds_add(&S.sc[SC_AD_A], S.cnt[1][tid]);
        lds_add(&S.sc[SC_AD_B], S.x[tid * SEG]);   // 256 values below 65521
    }
}

// ---- phases 3 and 5: the greedy choice at EVERY position of the segment, from its end backwards (the run lengths of both
// candidates are carried along).  TOK = false: x[p] = where the chain of tokens starting at p leaves the segment.
// TOK = true: x[p] = the token at p: length 1 (a literal) or 3..258, bit 15 = the candidate.
// The fixed rule: the longer of the two candidates' runs, cut at 258 and at the chunk's end; the sample distance on a tie; a
// literal below 3.
template <bool TOK>
HKD_FN void phase_parse(Shared& S, const Chunk& c, int tid) {
    const int p0 = tid * SEG;
    if (p0 >= c.n) return;
    const int p1 = p0 + SEG < c.n ? p0 + SEG : c.n;
    int r[2];
    for (int k = 0; k < 2; ++k) {
        int nz = tid + 1 < THREADS ? (int)S.fz[0][k][tid + 1] : c.n;
        nz = nz < c.n ? nz : c.n;
        r[k] = nz - p1;
    }
    int r0 = r[0], r1 = r[1];
    for (int p = p1 - 1; p >= p0; --p) {
        r0 = eq(S, c, 0, p) ? r0 + 1 : 0;
        r1 = eq(S, c, 1, p) ? r1 + 1 : 0;
        const int l0 = r0 < 258 ? r0 : 258, l1 = r1 < 258 ? r1 : 258;
        int len = l1 > l0 ? l1 : l0;
        const int sel = l1 > l0 ? 1 : 0;
        if (len < 3) len = 1;
        if (TOK) {
            S.x[p] = (unsigned short)(len | (sel << 15));
        } else {
            const int nx = p + len;
            S.x[p] = nx >= p1 ? (unsigned short)nx : S.x[nx];
        }
    }
}

// ---- phase 4 (one lane): the token chain from byte 0 visits each segment once: where it enters
HKD_FN void phase_walk(Shared& S, const Chunk& c, int tid) {
    if (tid != 0) return;
    int pos = 0;
    for (int t = 0; t < THREADS && pos < c.n; ++t)
        if (pos < (t + 1) * SEG) {
            S.entry[t] = (unsigned short)pos;
            pos = S.x[pos];
        }
}

// ---- phase 6: symbol counts of the tokens that start in the segment
HKD_FN void phase_count(Shared& S, const Chunk& c, int tid) {
    if (tid == 0) S.hll[256] = 1;   // (nothing else counts the end-of-block symbol)
    int p = S.entry[tid];
    if (p == (int)NONE) return;
    const int p1 = (tid + 1) * SEG < c.n ? (tid + 1) * SEG : c.n;
    while (p < p1) {
        const unsigned t = S.x[p];
        const int len = (int)(t & 0x7FFF);
        if (len == 1) {
            lds_add(&S.hll[S.data[HIST + p]], 1);
        } else {
            int code, ext, extv;
            length_code(len, code, ext, extv);
            lds_add(&S.hll[257 + code], 1);
            lds_add(&S.hd[c.dcode((int)(t >> 15))], 1);
        }
        p += len;
    }
}

// ---- code construction --------------------------------------------------------------------------------------------------
// rank of every used symbol among the used ones by (count, symbol): key / sym in ascending order
HKD_FN void rank_sort(Shared& S, const unsigned* h, int n, int tid) {
    for (int s = tid; s < n; s += THREADS) {
        const unsigned f = h[s];
        if (f == 0) continue;
        int rank = 0;
        for (int o = 0; o < n; ++o) {
            const unsigned g = h[o];
            rank += (g != 0) & ((g < f) | ((g == f) & (o < s)));
        }
        S.key[rank] = f, S.sym[rank] = (unsigned short)s;
        lds_add(&S.sc[SC_NUSED], 1);
    }
}

// (one lane)  key[0..n) ascending counts, n >= 2 -> numc[l] = number of codes of length l, limited to `limit` bits.
// The in-place minimum-redundancy construction of Moffat and Katajainen, then the limit as zlib-style coders enforce it: fold the
// lengths above the limit into it and repair the Kraft sum by lengthening the deepest shorter code, one step at a time.
HKD_FN void code_lengths(Shared& S, int n, int limit) {
    unsigned* A = S.key;
    for (int i = 0; i <= MAXDEPTH; ++i) S.numc[i] = 0;
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) {
            A[next] = A[root];
            A[root++] = (unsigned)next;
        } else {
            A[next] = A[leaf++];
        }
        if (leaf >= n || (root < next && A[root] < A[leaf])) {
            A[next] += A[root];
            A[root++] = (unsigned)next;
        } else {
            A[next] += A[leaf++];
        }
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) ++used, --root;
        while (avbl > used) {
            S.numc[dpth < MAXDEPTH ? dpth : MAXDEPTH] += 1;
            --avbl;
        }
        avbl = 2 * used, ++dpth, used = 0;
    }
    for (int i = limit + 1; i <= MAXDEPTH; ++i) S.numc[limit] += S.numc[i], S.numc[i] = 0;
    unsigned total = 0;
    for (int i = limit; i > 0; --i) total += S.numc[i] << (limit - i);
    while (total != (1u << limit)) {
        S.numc[limit] -= 1;
        for (int i = limit - 1; i > 0; --i)
            if (S.numc[i]) {
                S.numc[i] -= 1, S.numc[i + 1] += 2;
                break;
            }
        --total;
    }
}

// (one lane)  lengths to the symbols, the rarest first and longest; first canonical code of every length
HKD_FN void assign_lengths(Shared& S, int n, int limit, unsigned char* len) {
    int j = n;
    for (int l = 1; l <= limit; ++l)
        for (unsigned k = S.numc[l]; k > 0; --k) len[S.sym[--j]] = (unsigned char)l;
    unsigned code = 0;
    S.first[0] = 0;
    for (int l = 1; l <= 15; ++l) {
        code = (code + (l - 1 <= limit ? S.numc[l - 1] : 0)) << 1;
        S.first[l] = code;
    }
}

// ---- phase 7a: order the literal/length symbols
HKD_FN void phase_sort_ll(Shared& S, int tid) { rank_sort(S, S.hll, NLL, tid); }

// ---- phase 7b: lane 0: literal/length code lengths (15 bits); lane 64: the distance code (at most two symbols: one bit each;
// none: one unused code of one bit, as zlib writes it)
HKD_FN void phase_lengths(Shared& S, const Chunk& c, int tid) {
    if (tid == 0) {
        const int n = (int)S.sc[SC_NUSED];   // >= 2: the end-of-block symbol and a literal or a length
        code_lengths(S, n, 15);
        assign_lengths(S, n, 15, S.lll);
        S.numc[0] = 0;
        int hlit = NLL;
        while (hlit > 257 && S.hll[hlit - 1] == 0) --hlit;
        S.sc[SC_HLIT] = (unsigned)hlit;
    }
    if (tid == 64 % THREADS) {
        const int c0 = c.dcode0, c1 = c.dcode1;   // c0 < c1
        const bool u0 = S.hd[c0] != 0, u1 = S.hd[c1] != 0;
        int hdist = 1;
        if (!u0 && !u1) {
            S.dl[0] = 1, S.dc[0] = 0;
        } else {
            if (u0) S.dl[c0] = 1, S.dc[c0] = 0, hdist = c0 + 1;
            if (u1) S.dl[c1] = 1, S.dc[c1] = u0 ? 1 : 0, hdist = c1 + 1;
        }
        S.sc[SC_HDIST] = (unsigned)hdist;
    }
}

// ---- phase 7c: all lanes: canonical literal/length codes and the body's size; lane 64 then writes the code-length header
HKD_FN void phase_codes(Shared& S, const Chunk& c, int tid) {
    unsigned bits = 0;
    for (int s = tid; s < NLL; s += THREADS) {
        const int l = S.lll[s];
        if (l == 0) continue;
        unsigned code = S.first[l];
        for (int o = 0; o < s; ++o) code += S.lll[o] == l;
        S.llc[s] = (unsigned short)(bitrev(code) >> (32 - l));
        bits += S.hll[s] * (unsigned)(l + ll_extra_bits(s));
    }
    if (tid < 2) bits += S.hd[c.dcode(tid)] * (unsigned)(S.dl[c.dcode(tid)] + c.dext(tid));
    if (bits) lds_add(&S.sc[SC_BODY], bits);
    if (tid != 64 % THREADS) return;
    // the HLIT + HDIST code lengths as one sequence of symbols 0..15 and repeats 16 (the last length 3..6 times), 17 (3..10 zeros),
    // 18 (11..138 zeros)
    for (int i = 0; i < NCL; ++i) S.hcl[i] = 0, S.cll[i] = 0, S.clc[i] = 0;
    const int hlit = (int)S.sc[SC_HLIT], total = hlit + (int)S.sc[SC_HDIST];
    int nr = 0, i = 0;
    while (i < total) {
        const int l = i < hlit ? S.lll[i] : S.dl[i - hlit];
        int run = 1;
        while (i + run < total && (i + run < hlit ? S.lll[i + run] : S.dl[i + run - hlit]) == l) ++run;
        i += run;
        if (l == 0) {
            while (run >= 11) {
                const int k = run < 138 ? run : 138;
                S.rsym[nr] = 18, S.rext[nr] = (unsigned char)(k - 11), ++nr, S.hcl[18] += 1, run -= k;
            }
            if (run >= 3) S.rsym[nr] = 17, S.rext[nr] = (unsigned char)(run - 3), ++nr, S.hcl[17] += 1, run = 0;
        } else {
            S.rsym[nr] = (unsigned char)l, S.rext[nr] = 0, ++nr, S.hcl[l] += 1, --run;
            while (run >= 3) {
                const int k = run < 6 ? run : 6;
                S.rsym[nr] = 16, S.rext[nr] = (unsigned char)(k - 3), ++nr, S.hcl[16] += 1, run -= k;
            }
        }
        for (; run > 0; --run) S.rsym[nr] = (unsigned char)l, S.rext[nr] = 0, ++nr, S.hcl[l] += 1;
    }
    S.sc[SC_NRLE] = (unsigned)nr;
    S.sc[SC_NUSED] = 0;
}

// ---- phase 7d: order the code-length symbols
HKD_FN void phase_sort_cl(Shared& S, int tid) { rank_sort(S, S.hcl, NCL, tid); }

// the order in which the header stores the code-length code's lengths
HKD_FN int cl_order(int i) {
    // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return i < 3 ? 16 + i : (i == 3 ? 0 : ((i & 1) ? 7 - ((i - 5) >> 1) : 8 + ((i - 4) >> 1)));
}

// ---- phase 7e (one lane): the code-length code (7 bits), the header's size, and the choice between the two forms
HKD_FN void phase_decide(Shared& S, const Chunk& c, int tid) {
    if (tid != 0) return;
    int n = (int)S.sc[SC_NUSED];
    if (n == 1) {   // a code of one symbol is not complete: give it a partner nothing uses
        const int s = S.sym[0];
        S.cll[s] = 1, S.cll[s == 0 ? 1 : 0] = 1;
    } else {
        code_lengths(S, n, 7);
        assign_lengths(S, n, 7, S.cll);
    }
    unsigned hdr = 3 + 5 + 5 + 4;
    // canonical codes of at most 19 symbols
    {
        unsigned cnt_l, code = 0;
        for (int l = 1; l <= 7; ++l) {
            cnt_l = 0;
            for (int s = 0; s < NCL; ++s)
                if (S.cll[s] == l) {
                    S.clc[s] = (unsigned short)(bitrev(code + cnt_l) >> (32 - l));
                    ++cnt_l;
                }
            code = (code + cnt_l) << 1;
        }
    }
    int hclen = NCL;
    while (hclen > 4 && S.cll[cl_order(hclen - 1)] == 0) --hclen;
    hdr += 3 * (unsigned)hclen;
    for (int s = 0; s < NCL; ++s) hdr += S.hcl[s] * (unsigned)(S.cll[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
    S.sc[SC_HCLEN] = (unsigned)hclen;
    S.sc[SC_HDR] = hdr;
    // the block's bits, the 3 header bits of the empty stored block, padding to a byte, its 4 length bytes
    const unsigned dyn = (hdr + S.sc[SC_BODY] + 3 + 7) / 8 + 4;
    S.sc[SC_DYN] = dyn < (unsigned)c.n + 5 ? dyn : 0;   // 0: the stored form
}

// ---- phase 8: the bits of the tokens that start in the segment (then an inclusive prefix sum over the segments, 8 rounds)
HKD_FN void phase_bits(Shared& S, const Chunk& c, int tid) {
    unsigned bits = 0;
    int p = S.entry[tid];
    if (p != (int)NONE) {
        const int p1 = (tid + 1) * SEG < c.n ? (tid + 1) * SEG : c.n;
        while (p < p1) {
            const unsigned t = S.x[p];
            const int len = (int)(t & 0x7FFF);
            if (len == 1) {
                bits += S.lll[S.data[HIST + p]];
            } else {
                int code, ext, extv;
                length_code(len, code, ext, extv);
                const int k = (int)(t >> 15);
                bits += (unsigned)(S.lll[257 + code] + ext + S.dl[c.dcode(k)] + c.dext(k));
            }
            p += len;
        }
    }
    S.cnt[0][tid] = bits;
}
HKD_FN void phase_bits_round(Shared& S, int tid, int r) {
    const int from = r & 1, to = from ^ 1, o = tid - (1 << r);
    S.cnt[to][tid] = S.cnt[from][tid] + (o >= 0 ? S.cnt[from][o] : 0);
}

// ---- phase 9: the block.  Lane 64 writes the header, every lane its segment's tokens, the last lane the end of the block and
// the empty stored block behind it.
HKD_FN void phase_emit(Shared& S, const Chunk& c, int tid) {
    const unsigned hdr = S.sc[SC_HDR];
    if (tid == 64 % THREADS) {
        unsigned pos = 0;
        put_bits(S, pos, 0u | (2u << 1), 3), pos += 3;   // BFINAL = 0, BTYPE = 10
        put_bits(S, pos, S.sc[SC_HLIT] - 257, 5), pos += 5;
        put_bits(S, pos, S.sc[SC_HDIST] - 1, 5), pos += 5;
        put_bits(S, pos, S.sc[SC_HCLEN] - 4, 4), pos += 4;
        for (int i = 0; i < (int)S.sc[SC_HCLEN]; ++i) put_bits(S, pos, S.cll[cl_order(i)], 3), pos += 3;
        for (int i = 0; i < (int)S.sc[SC_NRLE]; ++i) {
            const int s = S.rsym[i];
            put_bits(S, pos, S.clc[s], S.cll[s]), pos += S.cll[s];
            const int e = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
            put_bits(S, pos, S.rext[i], e), pos += (unsigned)e;
        }
    }
    unsigned pos = hdr + (tid ? S.cnt[0][tid - 1] : 0);
    int p = S.entry[tid];
    if (p != (int)NONE) {
        const int p1 = (tid + 1) * SEG < c.n ? (tid + 1) * SEG : c.n;
        while (p < p1) {
            const unsigned t = S.x[p];
            const int len = (int)(t & 0x7FFF);
            if (len == 1) {
                const int s = S.data[HIST + p];
                put_bits(S, pos, S.llc[s], S.lll[s]), pos += S.lll[s];
            } else {
                int code, ext, extv;
                length_code(len, code, ext, extv);
                const int k = (int)(t >> 15), s = 257 + code, dcd = c.dcode(k);
                put_bits(S, pos, S.llc[s], S.lll[s]), pos += S.lll[s];
                put_bits(S, pos, (unsigned)extv, ext), pos += (unsigned)ext;
                put_bits(S, pos, S.dc[dcd], S.dl[dcd]), pos += S.dl[dcd];
                put_bits(S, pos, (unsigned)c.dextv(k), c.dext(k)), pos += (unsigned)c.dext(k);
            }
            p += len;
        }
    }
    if (tid == THREADS - 1) {
        pos = hdr + S.cnt[0][THREADS - 1];
        put_bits(S, pos, S.llc[256], S.lll[256]), pos += S.lll[256];
        pos = (pos + 3 + 7) / 8 * 8;         // 000: not final, stored; padding
        put_bits(S, pos + 16, 0xFFFFu, 16);  // LEN = 0000, NLEN = FFFF
    }
}

// byte j of the stored form of the chunk
HKD_FN unsigned stored_byte(const Shared& S, const Chunk& c, int j) {
    const unsigned n = (unsigned)c.n, nn = ~n & 0xFFFFu;
    if (j >= 5) return j - 5 < c.n ? S.data[HIST + j - 5] : 0u;
    return j == 0 ? 0u : j == 1 ? (n & 0xFFu) : j == 2 ? ((n >> 8) & 0xFFu) : j == 3 ? (nn & 0xFFu) : (nn >> 8);
}

}  // namespace deflate
}  // namespace hk
