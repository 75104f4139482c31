// hk_deflate.hip -- the DEFLATE (zlib) streams of a tiled GeoTIFF's tiles, made on the device: what tiff.write_tiff otherwise gets
// from zlib.compress on one host thread, tile by tile.
//
// THE STREAM (the contract).  A tile's raw bytes are `tile` rows of `tile` little-endian samples, edge tiles
// zero-padded; tiles are ordered band, tile row, tile column.  The raw bytes are cut into chunks of HK_DEFLATE_CHUNK = 16384 (the
// last one of a tile may be shorter).  The tile's stream is
//   1. the zlib header 78 9C;
//   2. per chunk EITHER one dynamic-Huffman block (BTYPE = 10, not final) followed by an empty stored block (3 zero bits, padding
//      to the byte, 00 00 FF FF), so that every chunk starts and ends on a byte boundary, OR one stored block (00, LEN, NLEN, the
//      bytes) -- the stored block whenever the dynamic form with its marker would not be smaller than chunk + 5 bytes;
//   3. a final empty fixed block (03 00);
//   4. the Adler-32 of the raw bytes, big-endian.
// Tokens of a dynamic block are literals and matches of length 3..258 at one of TWO distances: the sample size (1, 2, 4, 8 bytes)
// and the tile's row length in bytes (tile x sample size <= 4096).  The parse is greedy and fixed: at a token start the longer of
// the two candidates' runs (cut at 258 and at the chunk's end) if it is at least 3, the sample distance on a tie, else a literal.  A
// match may reach back into the previous chunk of the tile, never in front of the tile's first byte.  No hash table, no search:
// rasters repeat the sample beside and the sample above, and these two candidates are the design.  Both Huffman codes are built per
// chunk from its own counts (15 bits at most; the code-length code 7 bits; repeat symbols 16 / 17 / 18 in the header).  Nothing
// depends on the order in which lanes or workgroups run: the same input gives the same bytes.
//
// deflate_chunk_kernel: one workgroup per chunk; hk_deflate_core.h holds its phases (and says how they are tested without a GPU).
// The chunk and 4096 bytes of history lie in LDS (16-byte loads); run lengths per candidate come from a per-byte equality and a
// suffix-minimum scan over the 256 segments; the greedy chain is found by composing per-segment "where does a chain that enters
// here leave" tables and one walk over the segments; counts are LDS atomics; the codes are built in LDS; the block's size is
// known, and the form chosen, before a bit is written; the bits are assembled in LDS at prefix-summed offsets and leave as 16-byte
// stores into the chunk's own slot of SLOT = 16400 bytes (chunk + 5 rounded up to 16: the stored form is the worst case).
// deflate_offsets_kernel (one workgroup): tile sizes and their even-aligned exclusive prefix sum.  deflate_gather_kernel (one
// workgroup per chunk): the slots compacted into contiguous tile streams, zlib header, final block and combined Adler-32.
// About 78 KiB of LDS per workgroup: two workgroups per CU.
//
// WITH A PREDICTOR (TIFF tag 317; launch_deflate_tiles(predictor, ...)) all of the above holds for the tile's PREDICTED bytes: the
// predictor runs over each zero-padded tile row on its own (deflate::predicted_byte in hk_deflate_core.h states both: 2, integer
// differences modulo the sample's width; 3, libtiff's floating-point predictor -- byte planes, most significant first, differenced
// modulo 256 over the whole row), the Adler-32 is taken over the predicted bytes, and the two candidate distances are the sample
// size and the row length with predictors 1 and 2, and ONE and the row length with predictor 3: the bytes of a plane repeat at
// distance 1.  Predictor 1 launches deflate_chunk_kernel and gives the bytes it always gave; 2 and 3 launch
// deflate_pred_chunk_kernel (hk_deflate_pred.hip), whose phase 0 stages the whole raw rows under the chunk and its history and predicts from LDS (why
// there and not in a pre-pass: DESIGN.md 5.4).
#include <hip/hip_runtime.h>

#include "hk_deflate_core.h"
#include "hk_kernels.h"

namespace hk {

namespace {

using namespace deflate;

typedef __attribute__((address_space(1))) const unsigned char g_cbyte;
typedef __attribute__((address_space(1))) unsigned char g_byte;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const u32x4 g_cuint4;
typedef __attribute__((address_space(1))) u32x4 g_uint4;
typedef __attribute__((address_space(1))) const unsigned g_cuint;
typedef __attribute__((address_space(1))) unsigned g_uint;
typedef __attribute__((address_space(1))) long long g_ll;
typedef __attribute__((address_space(1))) const long long g_cll;

__device__ __forceinline__ int chunk_bytes(int tile_bytes, int c) {
    const int left = tile_bytes - c * CHUNK;
    return left < CHUNK ? left : CHUNK;
}

}  // namespace

__global__ void __launch_bounds__(deflate::THREADS) deflate_chunk_kernel(const DeflateArgs a) {
    __shared__ Shared S;
    const int tid = threadIdx.x;
    const long long g = blockIdx.x;
    const int t = (int)(g / a.cpt), ci = (int)(g % a.cpt);
    const int band = t / (a.across * a.down), ty = (t / a.across) % a.down, tx = t % a.across;
    const int es = a.es, row_bytes = a.tile * es;
    const int start = ci * CHUNK, n = chunk_bytes(a.tile_bytes, ci);
    const Chunk c = make_chunk(start, n, es, row_bytes);

    // ---- phase 0: the chunk and its history into LDS, 16 bytes per lane and step (a group never straddles a tile row: the row
    // length is a multiple of 16 bytes); what lies outside the raster reads as zero
    {
        g_cbyte* const plane = (g_cbyte*)a.src + (long long)band * a.band_stride * es;
        const int hist = start < HIST ? start : HIST;
        const long long width_bytes = (long long)a.width * es;
        for (int k = (HIST - hist) / 16 + tid; k < (HIST + n) / 16; k += THREADS) {
            const int q = start - HIST + 16 * k;   // byte of the tile
            const int r = q / row_bytes, cb = q % row_bytes;
            const long long gy = (long long)ty * a.tile + r, gxb = (long long)tx * row_bytes + cb;
            g_cbyte* const p = plane + gy * a.stride * es + gxb;
            u32x4 v = {0, 0, 0, 0};
            if (gy < a.height && gxb < width_bytes) {
                if (a.vec_ok && gxb + 16 <= width_bytes) {
                    v = *(g_cuint4*)p;
                } else {
                    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (gxb + j < width_bytes) w[j >> 2] |= (unsigned)p[j] << (8 * (j & 3));
                    v = u32x4{w[0], w[1], w[2], w[3]};
                }
            }
            *reinterpret_cast<u32x4*>(&S.data[16 * k]) = v;
        }
    }
    __syncthreads();
    phase_scan(S, c, tid);
    __syncthreads();
    for (int r = 0; r < 8; ++r) {
        phase_scan_round(S, tid, r);
        __syncthreads();
    }
    phase_parse<false>(S, c, tid);
    __syncthreads();
    phase_walk(S, c, tid);
    __syncthreads();
    phase_parse<true>(S, c, tid);
    __syncthreads();
    phase_count(S, c, tid);
    __syncthreads();
    phase_sort_ll(S, tid);
    __syncthreads();
    phase_lengths(S, c, tid);
    __syncthreads();
    phase_codes(S, c, tid);
    __syncthreads();
    phase_sort_cl(S, tid);
    __syncthreads();
    phase_decide(S, c, tid);
    __syncthreads();
    const unsigned dyn = S.sc[SC_DYN];   // (uniform)
    if (dyn) {
        phase_bits(S, c, tid);
        __syncthreads();
        for (int r = 0; r < 8; ++r) {
            phase_bits_round(S, tid, r);
            __syncthreads();
        }
        phase_emit(S, c, tid);
        __syncthreads();
    }
    // ---- the slot: whole 16-byte words, at most SLOT bytes (dyn < n + 5 <= SLOT; the stored form is n + 5)
    const unsigned size = dyn ? dyn : (unsigned)n + 5;
    g_uint4* const slot = (g_uint4*)((g_byte*)a.slots + g * SLOT);
    for (int k = tid; k < (int)((size + 15) / 16); k += THREADS) {
        u32x4 v;
        if (dyn) {
            v = *reinterpret_cast<const u32x4*>(&S.out[4 * k]);
        } else {
            unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j >> 2] |= stored_byte(S, c, 16 * k + j) << (8 * (j & 3));
            v = u32x4{w[0], w[1], w[2], w[3]};
        }
        slot[k] = v;
    }
    if (tid == 0) {
        ((g_uint*)a.sizes)[g] = size;
        ((g_uint*)a.adler)[g] = (S.sc[SC_AD_A] % 65521u) | ((S.sc[SC_AD_B] % 65521u) << 16);
    }
}

// tile t: 2 + its chunks + 2 + 4 bytes; tile_offsets = exclusive prefix sum of the sizes rounded up to even; [n_tiles] = the total
__global__ void __launch_bounds__(256) deflate_offsets_kernel(const DeflateArgs a, int n_tiles, long long* tile_offsets,
                                                               long long* tile_sizes) {
    __shared__ long long scan[2][256];
    __shared__ long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int t0 = 0; t0 < n_tiles; t0 += 256) {
        const int t = t0 + tid;
        long long s = 0;
        if (t < n_tiles) {
            s = 8;
            for (int ci = 0; ci < a.cpt; ++ci) s += ((g_cuint*)a.sizes)[(long long)t * a.cpt + ci];
            ((g_ll*)tile_sizes)[t] = s;
            s += s & 1;
        }
        scan[0][tid] = s;
        __syncthreads();
        for (int r = 0; r < 8; ++r) {
            const int from = r & 1, o = tid - (1 << r);
            scan[from ^ 1][tid] = scan[from][tid] + (o >= 0 ? scan[from][o] : 0);
            __syncthreads();
        }
        const long long base = carry;
        if (t < n_tiles) ((g_ll*)tile_offsets)[t] = base + scan[0][tid] - s;
        __syncthreads();
        if (tid == 255) carry = base + scan[0][255];
        __syncthreads();
    }
    if (tid == 0) ((g_ll*)tile_offsets)[n_tiles] = carry;
}

// chunk g of tile t: its slot's bytes to their place in the tile's stream; the first chunk's workgroup adds the zlib header, the last
// one's the final block, the tile's Adler-32 and the padding byte of an odd stream
__global__ void __launch_bounds__(256) deflate_gather_kernel(const DeflateArgs a, const long long* tile_offsets, unsigned char* out) {
    const int tid = threadIdx.x;
    const long long g = blockIdx.x;
    const int t = (int)(g / a.cpt), ci = (int)(g % a.cpt);
    g_cuint* const sizes = (g_cuint*)a.sizes + (long long)t * a.cpt;
    const long long tile_at = ((g_cll*)tile_offsets)[t];
    long long before = 2;
    for (int k = 0; k < ci; ++k) before += sizes[k];
    const unsigned size = sizes[ci];
    g_byte* const dst = (g_byte*)out + tile_at + before;
    g_cbyte* const src = (g_cbyte*)a.slots + g * SLOT;
    // whole aligned words of the destination from two aligned words of the slot; the bytes around them one by one
    const unsigned head = (unsigned)((4 - ((unsigned long long)dst & 3)) & 3);
    const unsigned lead = head < size ? head : size;
    const unsigned words = (size - lead) / 4;
    for (unsigned i = tid; i < lead; i += 256) dst[i] = src[i];
    for (unsigned i = tid; i < (size - lead) % 4; i += 256) dst[lead + 4 * words + i] = src[lead + 4 * words + i];
    const unsigned sh = 8 * (lead & 3);
    g_cuint* const sw = (g_cuint*)(src + (lead & ~3u));   // (lead < 4: the slot's first word)
    g_uint* const dw = (g_uint*)(dst + lead);
    for (unsigned i = tid; i < words; i += 256) {
        const unsigned lo = sw[i];
        // word i + 1 of the slot exists whenever it is needed: it holds byte lead + 4 i + 4 > ... of the slot's `size` bytes
        dw[i] = sh ? (lo >> sh) | (sw[i + 1] << (32 - sh)) : lo;
    }
    if (tid == 0 && ci == 0) {
        g_byte* const h = (g_byte*)out + tile_at;
        h[0] = 0x78, h[1] = 0x9C;
    }
    if (tid == 0 && ci == a.cpt - 1) {
        unsigned s1 = 1, s2 = 0;
        g_cuint* const ad = (g_cuint*)a.adler + (long long)t * a.cpt;
        for (int k = 0; k < a.cpt; ++k) {
            const unsigned v = ad[k], nk = (unsigned)chunk_bytes(a.tile_bytes, k);
            s2 = (s2 + nk * s1 + (v >> 16)) % 65521u;   // nk * s1 < 2^14 * 2^16
            s1 = (s1 + (v & 0xFFFFu)) % 65521u;
        }
        g_byte* const e = dst + size;
        e[0] = 0x03, e[1] = 0x00;
        e[2] = (unsigned char)(s2 >> 8), e[3] = (unsigned char)s2, e[4] = (unsigned char)(s1 >> 8), e[5] = (unsigned char)s1;
        if ((before + size + 6) & 1) e[6] = 0;
    }
}

size_t deflate_workspace_bytes(long long n_chunks) {
    return (size_t)n_chunks * deflate::SLOT + ((size_t)n_chunks * 8 + 255) / 256 * 256;
}

hipError_t launch_deflate_tiles(int predictor, const DeflateTiles& r, void* work, hipStream_t stream) {
    const BandPlanes& p = r.planes;
    const int esize = r.esize, tile = r.tile;
    DeflateArgs a;
    memset(&a, 0, sizeof(a));
    a.src = p.src, a.es = esize, a.height = p.height, a.width = p.width, a.stride = p.stride, a.band_stride = p.band_stride;
    a.tile = tile, a.across = (p.width + tile - 1) / tile, a.down = (p.height + tile - 1) / tile;
    a.tile_bytes = tile * tile * esize, a.cpt = (a.tile_bytes + deflate::CHUNK - 1) / deflate::CHUNK;
    const long long n_tiles = (long long)p.n_bands * a.across * a.down, n_chunks = n_tiles * a.cpt;
    if (n_chunks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    a.vec_ok = ((uintptr_t)p.src % 16 == 0) && ((p.stride * esize) % 16 == 0) && ((p.band_stride * esize) % 16 == 0);
    a.slots = static_cast<unsigned char*>(work);
    a.sizes = reinterpret_cast<unsigned*>(a.slots + (size_t)n_chunks * deflate::SLOT);
    a.adler = a.sizes + n_chunks;
    hipError_t e;
    if (predictor == 1) {
        HK_LAUNCH(deflate_chunk_kernel, dim3((unsigned)n_chunks), dim3(deflate::THREADS), 0, stream, a);
        e = hipGetLastError();
    } else {
        e = launch_deflate_pred_chunks(a, predictor, n_chunks, stream);
    }
    if (e != hipSuccess) return e;
    HK_LAUNCH(deflate_offsets_kernel, dim3(1), dim3(256), 0, stream, a, (int)n_tiles, r.tile_offsets, r.tile_sizes);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    HK_LAUNCH(deflate_gather_kernel, dim3((unsigned)n_chunks), dim3(256), 0, stream, a, r.tile_offsets, r.out);
    return hipGetLastError();
}

}  // namespace hk
