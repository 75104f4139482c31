// hk_deflate_pred.hip -- deflate_chunk_kernel of hk_deflate.hip over the PREDICTED bytes of a tile (TIFF predictors 2 and 3): the
// stream contract is stated at the top of hk_deflate.hip, the predictors in hk_deflate_core.h (deflate::predicted_byte).  A
// translation unit of its own, so that hk_deflate.hip -- the predictor-1 path -- compiles to the code it always was: with both
// kernels in one module the compiler's output for deflate_chunk_kernel changed and the launch took 1 % longer
// (profiles/deflate.txt).  The phases behind phase 0 are the same functions of hk_deflate_core.h in the same order.
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

// 16 bytes of tile (band, ty, tx) from byte q of the tile on (q a multiple of 16: a group never straddles a tile row, the row
// length is a multiple of 16 bytes); what lies outside the raster reads as zero
__device__ __forceinline__ u32x4 load_tile16(const DeflateArgs& a, g_cbyte* plane, int ty, int tx, int q) {
    const int row_bytes = a.tile * a.es;
    const long long width_bytes = (long long)a.width * a.es;
    const int r = q / row_bytes, cb = q % row_bytes;
    const long long gy = (long long)ty * a.tile + r, gxb = (long long)tx * row_bytes + cb;
    g_cbyte* const p = plane + gy * a.stride * a.es + gxb;
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
    return v;
}

// everything behind phase 0: S.data holds the chunk's bytes and its history
__device__ __forceinline__ void encode_chunk(Shared& S, const Chunk& c, const DeflateArgs& a, long long g, int tid) {
    const int n = c.n;
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

}  // namespace

// deflate_chunk_kernel over the PREDICTED bytes of the tile (`predictor` 2 or 3; deflate::predicted_byte).  A predicted byte
// needs up to 2 es raw bytes of its own row, and a chunk boundary may fall inside a row, so phase 0 has two steps: (a) the WHOLE
// raw rows that the chunk and its history touch into LDS, 16 bytes per lane and step as above -- they lie in S.x, which no phase
// reads before phase 1 writes it, and are at most HIST + CHUNK + two rows = 28672 of its 32768 bytes; (b) every lane four
// predicted bytes per step, one dword store into S.data.  From there on the chunk is coded as ever.
__global__ void __launch_bounds__(deflate::THREADS) deflate_pred_chunk_kernel(const DeflateArgs a, const int predictor) {
    __shared__ Shared S;
    static_assert(sizeof(Shared::x) >= HIST + CHUNK + 2 * HIST, "the raw rows of a chunk and its history fit into x");
    const int tid = threadIdx.x;
    const long long g = blockIdx.x;
    const int t = (int)(g / a.cpt), ci = (int)(g % a.cpt);
    const int band = t / (a.across * a.down), ty = (t / a.across) % a.down, tx = t % a.across;
    const int es = a.es, row_bytes = a.tile * es;
    const int start = ci * CHUNK, n = chunk_bytes(a.tile_bytes, ci);
    const Chunk c = make_chunk(start, n, predictor_distance(predictor, es), row_bytes);
    const int hist = start < HIST ? start : HIST;
    const int first = start - hist;                                  // first byte of the tile that is staged
    const int r_lo = first / row_bytes, r_hi = (start + n - 1) / row_bytes;
    unsigned char* const raw = reinterpret_cast<unsigned char*>(S.x);   // rows r_lo .. r_hi of the tile
    {
        g_cbyte* const plane = (g_cbyte*)a.src + (long long)band * a.band_stride * es;
        for (int k = tid; k < (r_hi - r_lo + 1) * row_bytes / 16; k += THREADS)
            *reinterpret_cast<u32x4*>(&raw[16 * k]) = load_tile16(a, plane, ty, tx, r_lo * row_bytes + 16 * k);
    }
    __syncthreads();
    for (int k = (HIST - hist) / 4 + tid; k < (HIST + n) / 4; k += THREADS) {
        const int q = start - HIST + 4 * k;   // byte of the tile; its four bytes lie in one row (and one plane of predictor 3)
        const int r = q / row_bytes, j = q - r * row_bytes;
        const unsigned char* const row = raw + (r - r_lo) * row_bytes;
        unsigned w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) w |= predicted_byte(row, j + b, es, a.tile, predictor) << (8 * b);
        *reinterpret_cast<unsigned*>(&S.data[4 * k]) = w;
    }
    __syncthreads();
    encode_chunk(S, c, a, g, tid);
}

hipError_t launch_deflate_pred_chunks(const DeflateArgs& a, int predictor, long long n_chunks, hipStream_t stream) {
    HK_LAUNCH(deflate_pred_chunk_kernel, dim3((unsigned)n_chunks), dim3(deflate::THREADS), 0, stream, a, predictor);
    return hipGetLastError();
}

}  // namespace hk
