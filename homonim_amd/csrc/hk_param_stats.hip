// hk_param_stats.hip -- the masked per-band statistics behind homonim/stats.py:217-229 (ParamStats.stats, get_block_sums) and
// the data window of stats.py:135-173: per band, over the pixels valid under (nodata_mode, nodata),
//     [ min, max, sum x, sum x^2, N, N(x < thresh), col_min, row_min, col_max, row_max ]      (PARAM_STATS_N float64 values).
// The reference reads the file as float64 (out_dtype='float64') and lets numpy reduce it; here every pixel term is (double)x and
// (double)x * (double)x -- the square of a float32 is exact in float64 -- accumulated in float64 in a fixed order, so the
// result is bit-identical run to run.  min / max are the float32 values themselves, the counts are 64-bit integers (returned as
// doubles < 2^53), `x < thresh` is decided in float64 as numpy decides it (a NaN thresh counts nothing).  +-inf pixels are data.
// Under HK_NODATA_NONE / HK_NODATA_VALUE a NaN pixel is valid and makes min, max and both sums NaN, as it does in numpy: the
// kernels find that out from sum x^2, which is NaN exactly when a valid pixel was (x^2 >= 0: infinities alone never cancel).
//
// HBM-bound reduction: 4 bytes read per pixel*band, nothing written but the partials.  One pass; grid = PSTATS_BLOCKS x bands,
// each workgroup walks whole rows with 16-byte loads, wave butterfly + LDS across the four waves, one partial per workgroup; a
// second one-wave kernel per band combines the partials in index order.  Which thread reduces which pixel, and in which order,
// does not depend on whether the 16-byte loads are legal (the scalar path walks the same quads), so a plane gives the same bits
// through the host-pointer entry point (staged into an aligned slab) and the device-resident one (the caller's strides).
#include <hip/hip_runtime.h>

#include "hk_kernels.h"

namespace hk {

namespace {

constexpr int PSTATS_THREADS = 256;
constexpr int PSTATS_BLOCKS = 2048;  // workgroups per band (8 per CU)
constexpr int NP = PARAM_STATS_N;
constexpr int BOX_NONE = 0x7fffffff;

// validity as `cvalid` of hk_compare.hip decides it; the mode is a template argument here, so that the pixel loop holds no
// branch on it (as a run-time value the compiler turns the selection into scalar branches around every pixel, and those
// serialise the two loads the loop keeps in flight)
template <int MODE>
__device__ __forceinline__ bool pvalid(float v, float nodata) {
    return MODE == 0 ? true : (MODE == 1 ? !(v != v) : !(v == nodata));
}

// how value k of the vector combines: 0 min, 1 max, 2 sum
__device__ __forceinline__ int combine_op(int k) { return (k == 0 || k == 6 || k == 7) ? 0 : ((k == 1 || k == 8 || k == 9) ? 1 : 2); }

__device__ __forceinline__ double combine(int op, double a, double b) { return op == 0 ? fmin(a, b) : (op == 1 ? fmax(a, b) : a + b); }

__device__ __forceinline__ double wave_combine_f64(int op, double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = combine(op, v, __shfl_xor(v, off, 64));
    return v;
}

struct PAcc {
    float mn = __builtin_inff(), mx = -__builtin_inff();
    double s = 0.0, s2 = 0.0;
    unsigned n = 0, nb = 0;       // of the current row (folded into 64-bit totals after every row)
    int cmin = BOX_NONE, cmax = -1;
    template <int MODE>
    __device__ __forceinline__ void add(float x, int col, bool m, double thresh) {
        // fminf / fmaxf pass over a NaN operand: under NaN nodata a masked pixel needs no replacing (and a VALID NaN pixel of
        // the other modes leaves min / max to the final kernel, which knows of it from sum x^2)
        mn = fminf(mn, (MODE == 1 || m) ? x : __builtin_inff());
        mx = fmaxf(mx, (MODE == 1 || m) ? x : -__builtin_inff());
        const double d = (double)(m ? x : 0.f);  // masked pixels add zeros
        s += d, s2 += d * d;
        n += m ? 1u : 0u;
        nb += (m & (d < thresh)) ? 1u : 0u;
        cmin = min(cmin, m ? col : BOX_NONE);
        cmax = m ? col : cmax;                   // a thread's columns only grow along a row; rows are folded with max below
    }
};

template <int MODE, bool VEC>
__device__ __forceinline__ void walk_rows(const ParamStatsArgs& a, const float* __restrict__ plane, PAcc& acc,
                                          unsigned long long& n_total, unsigned long long& nb_total, int& rmin, int& rmax,
                                          int& cmax_all) {
    const int wq = a.width / 4;  // whole 4-pixel groups; rows are 16-byte aligned when VEC
    for (int y = blockIdx.x; y < a.height; y += gridDim.x) {
        const float* __restrict__ row = plane + (long long)y * a.stride;
        acc.cmax = -1;
#pragma unroll 2
        for (int q = threadIdx.x; q < wq; q += PSTATS_THREADS) {
            float v[4];
            if (VEC) {
                const float4 t = reinterpret_cast<const float4*>(row)[q];
                v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = row[4 * q + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc.add<MODE>(v[i], 4 * q + i, pvalid<MODE>(v[i], a.nodata), a.thresh);
        }
        for (int x = wq * 4 + threadIdx.x; x < a.width; x += PSTATS_THREADS) {
            const float v = row[x];
            acc.add<MODE>(v, x, pvalid<MODE>(v, a.nodata), a.thresh);
        }
        if (acc.n) rmin = min(rmin, y), rmax = y;  // a workgroup's rows only grow
        cmax_all = max(cmax_all, acc.cmax);
        n_total += acc.n, nb_total += acc.nb, acc.n = 0, acc.nb = 0;  // a row of one thread holds < 2^32 pixels
    }
}

}  // namespace

size_t param_stats_workspace_bytes(int n_bands) { return (size_t)n_bands * PSTATS_BLOCKS * NP * sizeof(double); }

// 8 waves per SIMD: left alone the compiler keeps both quads of the unrolled loop in registers (87 VGPRs, 5 waves per SIMD),
// which measured 4 % slower than the 48-register build (profiles/param_stats.txt)
template <int MODE>  // nodata mode: 0 none, 1 NaN, 2 value
__global__ void __launch_bounds__(PSTATS_THREADS, 8) param_stats_partial_kernel(const ParamStatsArgs a, double* __restrict__ partials) {
    const int band = blockIdx.y;
    const float* __restrict__ plane = a.planes + (long long)band * a.band_stride;
    PAcc acc;
    unsigned long long n_total = 0, nb_total = 0;
    int rmin = BOX_NONE, rmax = -1, cmax_all = -1;
    if (a.vec_ok)
        walk_rows<MODE, true>(a, plane, acc, n_total, nb_total, rmin, rmax, cmax_all);
    else
        walk_rows<MODE, false>(a, plane, acc, n_total, nb_total, rmin, rmax, cmax_all);
    // a thread without a valid pixel carries the empty band's box: [width, height, -1, -1]
    double v[NP] = {(double)acc.mn, (double)acc.mx, acc.s, acc.s2, (double)n_total, (double)nb_total,  // counts < 2^53: exact
                    (double)(acc.cmin == BOX_NONE ? a.width : acc.cmin), (double)(rmin == BOX_NONE ? a.height : rmin),
                    (double)cmax_all, (double)rmax};
    __shared__ double red[PSTATS_THREADS / 64][NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) v[k] = wave_combine_f64(combine_op(k), v[k]);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NP; ++k) red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NP) {
        const int op = combine_op(threadIdx.x);
        double t = red[0][threadIdx.x];
        for (int w = 1; w < PSTATS_THREADS / 64; ++w) t = combine(op, t, red[w][threadIdx.x]);
        partials[((size_t)band * gridDim.x + blockIdx.x) * NP + threadIdx.x] = t;
    }
}

__global__ void __launch_bounds__(64) param_stats_final_kernel(const double* __restrict__ partials, int n_partials, int height,
                                                                int width, double* __restrict__ stats_out) {
    const int band = blockIdx.x;
    const double* __restrict__ p = partials + (size_t)band * n_partials * NP;
    const double inf = __builtin_inf();
    double v[NP] = {inf, -inf, 0, 0, 0, 0, (double)width, (double)height, -1, -1};
    for (int i = threadIdx.x; i < n_partials; i += 64) {
#pragma unroll
        for (int k = 0; k < NP; ++k) v[k] = combine(combine_op(k), v[k], p[(size_t)i * NP + k]);
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) v[k] = wave_combine_f64(combine_op(k), v[k]);
    if (v[3] != v[3]) v[0] = v[1] = v[3];  // a valid NaN pixel (see the head of this file): min and max are NaN as well
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NP; ++k) stats_out[band * NP + k] = v[k];
    }
}

hipError_t launch_param_stats(const ParamStatsArgs& a_in, void* workspace, double* stats_out, hipStream_t stream) {
    ParamStatsArgs a = a_in;
    a.vec_ok = ((a.stride | a.band_stride) % 4 == 0) && (((uintptr_t)a.planes) % 16 == 0);
    const int blocks = a.height < PSTATS_BLOCKS ? a.height : PSTATS_BLOCKS;
    double* partials = static_cast<double*>(workspace);
    const dim3 grid(blocks, a.n_bands), block(PSTATS_THREADS);
    if (a.nd_mode == 0)
        HK_LAUNCH(param_stats_partial_kernel<0>, grid, block, 0, stream, a, partials);
    else if (a.nd_mode == 1)
        HK_LAUNCH(param_stats_partial_kernel<1>, grid, block, 0, stream, a, partials);
    else
        HK_LAUNCH(param_stats_partial_kernel<2>, grid, block, 0, stream, a, partials);
    HK_LAUNCH(param_stats_final_kernel, dim3(a.n_bands), dim3(64), 0, stream, partials, blocks, a.height, a.width, stats_out);
    return hipGetLastError();
}

}  // namespace hk
