// hk_kernels.h -- launch interface between the C-ABI host layer (hk_api.hip) and the gfx950 kernels (hk_fit_kernel.h: the fused kernel; hk_kernels.hip: its dispatch, apply, synthetic data, self-test).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "hk_layout.h"  // where the pieces of the in-painting's and the block statistics' workspaces lie; SlabLayout

struct hk_warp_desc;         // include/homonim_hk.h
struct hk_affine_warp_desc;  // include/homonim_hk.h

namespace hk {

constexpr int PX = 4;      // pixels per lane per row (one 16-byte load)
constexpr int WAVE = 64;   // gfx950 wavefront

// ---------------------------------------------------------------------------------------------------------------------
// Launch ledger (test aid; include/homonim_hk_devtools.h hk_debug_build_ledger).  Every kernel BUILD of the library -- each
// instantiation of the fused kernel's template, each kernel of the other translation units -- owns one BuildRecord that puts
// itself on a process-wide list when the library is loaded (so a build nothing ever launched is on the list too) and counts
// its launches.  The test-suite reads the list around every test and keeps a ledger of which builds were launched by a test
// that compared its results with the oracle (tests/conftest.py, tests/test_zz_build_ledger.py).  One relaxed atomic add per launch.
struct FitBuild;
struct BuildRecord {
    char name[88];
    unsigned long long launches;  // (atomic adds; read by ledger_text)
    BuildRecord* next;
    explicit BuildRecord(const char* kernel_name);
    explicit BuildRecord(const FitBuild& build);  // a build of the fused kernel, under fit_build_name()
    void hit() { __atomic_fetch_add(&launches, 1ull, __ATOMIC_RELAXED); }
};
// one record per launch SITE of a kernel outside the fused template: the site's local tag type names the kernel
template <typename Tag>
struct SiteRecord {
    static BuildRecord rec;
};
template <typename Tag>
BuildRecord SiteRecord<Tag>::rec{Tag::name()};
#define HK_LAUNCH(kern, ...)                                               \
    do {                                                                   \
        struct Tag_ {                                                      \
            static const char* name() { return #kern; }                    \
        };                                                                 \
        ::hk::SiteRecord<Tag_>::rec.hit();                                 \
        hipLaunchKernelGGL(kern, __VA_ARGS__);                             \
    } while (0)
// "name\tlaunches\n" per record, '\0'-terminated; returns the bytes needed (incl. the terminator) whatever `len` is
size_t ledger_text(char* buf, size_t len, bool reset);

// One job of a BATCHED launch (FitArgs::jobs, device memory): many device-resident jobs -- the block positions of a mosaic, the
// tiles of a tile list -- run as ONE kernel launch instead of one launch (and one launch tail) each.  A workgroup finds its job
// by a binary search over `first_group` and takes the job's planes, shape and unit grid from here instead of from FitArgs.
struct FitJob {
    const float* src;
    const float* ref;
    float* gain;
    float* offset;
    float* r2;
    float* corr;
    const double* norm;
    unsigned long long* fail_count;
    unsigned char* flag;
    long long stride, band_stride;
    int height, width, n_bands;
    int seg_rows, n_strips, n_segs, seg_rows_tail, n_segs_big;
    int out_y0, out_y1, out_x0, out_x1;
    int first_group[2];  // first workgroup of the job in the launch: [0] one strip per workgroup, [1] WPB_MEM strips (lock-step builds)
    int pad_;
};
static_assert(sizeof(FitJob) % 8 == 0, "FitJob entries are read with scalar loads");

// Device-side argument block of the fused fit(+apply) kernel.  One wave = one (band, row-segment, column-strip) unit.
struct FitArgs {
    const FitJob* jobs;     // batched launch: n_jobs entries (device), else NULL -- the fields below then describe the one job
    int n_jobs;
    int batch_groups[2];    // batched launch: workgroups of all jobs, [0] one strip per workgroup, [1] WPB_MEM strips
    const float* src;
    const float* ref;
    float* gain;
    float* offset;
    float* r2;
    float* corr;
    const double* norm;              // n_bands x 2 (gain-blk-offset)
    const float* offset_in;          // closing (in-paint) pass of gain-offset: in-painted offsets, else NULL
    const unsigned char* flag_in;    // ... with the source flags of the in-painting (1 byte per pixel): the build WITHOUT R2 then
                                     // takes the r2-mask decision from them instead of evaluating R2 again; else NULL
    unsigned long long* fail_count;  // n_bands
    unsigned char* flag;             // gain-offset with a threshold: 1 byte per pixel = 1: (r2 > thresh) & (gain > 0) & valid, 0: valid and failing, 2: invalid
                                     // (kernel_model.py:363), the in-painting's source mask; same strides as the planes; or NULL
    int height, width;
    long long stride;       // elements between rows
    long long band_stride;  // elements between planes
    int n_bands;
    int seg_rows;           // output rows per unit
    int n_strips, n_segs;   // units per band = n_strips * n_segs
    int seg_rows_tail;      // rows per unit of the last segments (launched last: they level the end of the launch)
    int n_segs_big;         // segments of seg_rows rows; the remaining n_segs - n_segs_big have seg_rows_tail rows
    int total_units;
    int rh, rw;             // kernel radii (kh = 2*rh+1, kw = 2*rw+1)
    int overlap_lanes;      // lanes per side that only feed neighbours: ceil(rw / PX)
    int src_nd_mode, ref_nd_mode;
    float src_nodata, ref_nodata;
    int has_thresh;
    float r2_thresh;
    int cert_only;          // gain-offset + r2 mask, no R2 plane, fail_count and open_rows set: run the CERTIFICATE build
                            // (choose_fit_build), which settles a wave-row by the two-sided float32 certificate or marks it in `open_rows`
    // The wave-rows the certificate build cannot settle: one bit per (band, strip, row), 32 rows per word, word index
    // (band * n_strips + strip) * ceil(height / 32) + row / 32 (zeroed before the certificate launch).
    // list_mode != 0: THIS launch is the list launch -- the complete build on a persistent grid over the runs of marked rows.
    unsigned* open_rows;
    int list_mode;
    float r2_fail_scale;    // kappa of the division-free r2-mask certificate: 1 - r2_pass_scale(), rounded up (hk_api.hip)
    float r2_failcert_scale;  // kappa_f of its mirror image (certain FAILURE; complete build): 1 - r2_fail_above(), rounded down; -inf: none
    double r2_pass_below;   // exact evaluation without R2 output: ssres < r2_pass_below * sstot proves the r2 test true,
    double r2_fail_above;   // ssres > r2_fail_above * sstot proves it false (sstot > 0); in between the division decides
    float n_full;           // kh * kw: the window count of every pixel away from the raster's edges (dense kernels)
    double nd_full;         // the same as float64
    double inv_n_full;      // RN64(1 / (kh * kw)) -- the 1/N table entry (hk_fit_kernel.h)
    int force_general;      // 1: never take the dense (nodata None) specialisation (testing)
    int seg_rows_pref;      // > 0: the build's preferred uniform segment height (hk_api.hip fill_args / fill_grid), 0: the default policy
    int use_ring;           // the ring mode ASKED for (hk_api.hip fill_args): 1 full LDS ring, 2 centre ring + re-loaded leaving row,
                            // 3 split ring (registers + LDS), 0 re-load both; choose_fit_build() resolves it to the ring that RUNS
    int xcd_remap;          // G > 0: blockIdx -> unit remap handing each XCD runs of G consecutive units (0: round-robin)
    int lds_pad;            // unused dynamic LDS bytes per wave: fewer resident waves per CU (hk_api.hip fill_args)
    // store window: only rows [out_y0, out_y1) x columns [out_x0, out_x1) of the job are written / counted (the halo crop of
    // homonim/raster_array.py:478-491 when a block of a larger device raster is processed in place); 0,height,0,width = all.
    // out_x0 and out_x1 are multiples of PX (or out_x1 == width): whole quads are stored.
    int out_y0, out_y1, out_x0, out_x1;
};

// The batched launch's table entry of one job from the job's own argument block (fill_args + fill_grid done); first_group
// is left to the caller
inline void fit_job_of(FitJob& e, const FitArgs& a) {
    memset(&e, 0, sizeof(e));
    e.src = a.src, e.ref = a.ref, e.gain = a.gain, e.offset = a.offset, e.r2 = a.r2, e.corr = a.corr, e.norm = a.norm;
    e.fail_count = a.fail_count, e.flag = a.flag;
    e.stride = a.stride, e.band_stride = a.band_stride, e.height = a.height, e.width = a.width, e.n_bands = a.n_bands;
    e.seg_rows = a.seg_rows, e.n_strips = a.n_strips, e.n_segs = a.n_segs, e.seg_rows_tail = a.seg_rows_tail;
    e.n_segs_big = a.n_segs_big;
    e.out_y0 = a.out_y0, e.out_y1 = a.out_y1, e.out_x0 = a.out_x0, e.out_x1 = a.out_x1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Which build of the fused kernel a launch gets.  A build is one instantiation of fit_apply_kernel<MODEL, R2, RW, DENSE, RING,
// CERT_ONLY, WPB, BATCH> or, `list`, of fit_list_kernel<MODEL, R2, RW, DENSE, RING> (hk_fit_kernel.h, which explains the
// parameters).  fit_build_exists() is the one statement of which are instantiated, choose_fit_build() the one place that picks
// one for a launch, launch_fit_build() (hk_fit_kernel.h) the one table that instantiates and launches them.
struct FitBuild {
    int model;       // 0 gain, 1 gain-blk-offset, 2 gain-offset
    bool r2;         // with the R2 quantity set
    int rw;          // kernel half-width 0..7; -1 - E: wider, half-width 4 F + E; -5 - E: the same with the whole lanes summed as pairs
    bool dense;      // both rasters have nodata None
    int ring;        // the ring mode that runs (FitArgs::use_ring is the one asked for)
    bool cert_only;  // the certificate build of gain-offset with the r2 mask
    int wpb;         // strips per workgroup: 1, or WPB_MEM in lock-step; 0: no build (choose_fit_build refused the launch)
    bool batch;      // with the job-table look-up of a batched launch (FitArgs::jobs)
    bool list;       // the list launch's kernel: the complete build over the rows the certificate build marked
};
constexpr int WPB_MEM = 4;  // strips per workgroup of the lock-step builds (hk_fit_kernel.h; FitJob::first_group[1] counts those)
// Register rows of the split ring (ring mode 3) a build holds = the largest kernel half-height it serves.
constexpr int SPLIT_RING_ROWS = 7, SPLIT_RING_ROWS_BLK = 5;  // (_BLK: the gain-blk-offset builds)
__host__ __device__ constexpr int split_ring_rows(int model) { return model == 1 ? SPLIT_RING_ROWS_BLK : SPLIT_RING_ROWS; }
// The builds with the job-table look-up: gain-blk-offset without R2 -- the fused RasterFuse path of a block-partitioned mosaic,
// where one launch for all blocks pays (profiles/r03_batch.txt).  The batched entry points run every other model as one launch
// per job (bit-identical either way).
constexpr bool fit_batch_build(int model, bool with_r2) { return model == 1 && !with_r2; }
// The full-ring builds that read the leaving row one iteration ahead (their ring holds a row less): the memory-bound ones
__host__ __device__ constexpr bool fit_ring_ahead(int model, bool r2, int ring) { return ring == 1 && model != 2 && !r2; }

constexpr bool fit_build_exists(int model, bool r2, int rw, bool dense, int ring, bool cert_only, int wpb, bool batch, bool list) {
    [[maybe_unused]] const bool mem_bound = model != 2 && !r2;  // gain, gain-blk-offset without the R2 work
    // kernel width x ring mode: the full ring up to 7 wide (the memory-bound builds: up to 15), the split ring 5 - 15 wide on the
    // memory-bound builds, everything re-loaded on the wide builds only, the centre ring at every width (wide: plain and paired)
#if defined(HK_DEV_SUBSET) && defined(HK_DEV_SUBSET15)  // development: only the 15-wide kernels with the centre / split ring
    const bool shape = rw == 7 && (ring == 2 || (ring == 3 && mem_bound));
#elif defined(HK_DEV_SUBSET)                             // development: only the 5x5 kernels with the full LDS ring
    const bool shape = rw == 2 && ring == 1;
#else
    const bool shape = ring == 1 ? rw >= 0 && rw <= (mem_bound ? 7 : 3)
                     : ring == 3 ? mem_bound && rw >= 2 && rw <= 7
                     : ring == 0 ? rw >= -4 && rw <= -1
                                 : ring == 2 && rw >= -8 && rw <= 7;
#endif
    if (model < 0 || model > 2 || !shape) return false;
    if (dense && model == 1) return false;  // gain-blk-offset's mask depends on the normalised values
    // certificate and list: gain-offset with the R2 work on the full and the centre ring, single waves, never batched
    if ((cert_only || list) && !(model == 2 && r2 && (ring == 1 || ring == 2) && wpb == 1 && !batch && !(cert_only && list))) return false;
    if (batch && !fit_batch_build(model, r2)) return false;
    // lock-step workgroups: every build without the R2 work on the full ring (gain-offset without a threshold gains 3 % as well)
    return wpb == 1 || (wpb == WPB_MEM && !r2 && ring == 1);
}
constexpr bool fit_build_exists(const FitBuild& b) {
    return fit_build_exists(b.model, b.r2, b.rw, b.dense, b.ring, b.cert_only, b.wpb, b.batch, b.list);
}
// The build for the launch `a` describes -- a.cert_only: the certificate build, a.list_mode: the list launch, a.jobs: batched --
// or, where that launch has no build (a certificate or list launch whose planes or ring have none, a job table on a model
// without the look-up), one with wpb == 0.  Plain host arithmetic.
FitBuild choose_fit_build(const FitArgs& a, int model, bool r2);
// "fit_apply_kernel<MODEL,R2,RW,DENSE,RING,CERT_ONLY,WPB,BATCH>" / "fit_list_kernel<MODEL,R2,RW,DENSE,RING>": the ledger's name
void fit_build_name(char* buf, size_t len, const FitBuild& b);
// choose_fit_build() + the launch; hipErrorInvalidValue where there is no build
hipError_t launch_fit_apply(const FitArgs& a, int model, bool with_r2, hipStream_t stream);
// ... through the table of the build's translation unit, one per (model, with_r2) (hk_fit_tu.hip)
hipError_t launch_fit_m0_r0(const FitBuild& b, const FitArgs& a, hipStream_t stream);
hipError_t launch_fit_m0_r1(const FitBuild& b, const FitArgs& a, hipStream_t stream);
hipError_t launch_fit_m1_r0(const FitBuild& b, const FitArgs& a, hipStream_t stream);
hipError_t launch_fit_m1_r1(const FitBuild& b, const FitArgs& a, hipStream_t stream);
hipError_t launch_fit_m2_r0(const FitBuild& b, const FitArgs& a, hipStream_t stream);
hipError_t launch_fit_m2_r1(const FitBuild& b, const FitArgs& a, hipStream_t stream);
hipError_t read_stamps_m0_r0(unsigned long long* acc16, bool reset);
hipError_t read_stamps_m0_r1(unsigned long long* acc16, bool reset);
hipError_t read_stamps_m1_r0(unsigned long long* acc16, bool reset);
hipError_t read_stamps_m1_r1(unsigned long long* acc16, bool reset);
hipError_t read_stamps_m2_r0(unsigned long long* acc16, bool reset);
hipError_t read_stamps_m2_r1(unsigned long long* acc16, bool reset);
// stage stamps of a -DHK_STAMPS build of the fused kernel (all zero otherwise): 16 counters, optionally cleared after reading
hipError_t read_stamps(unsigned long long* out16, bool reset);
// lanes per side that overlap with the neighbouring strip for kernel half-width rw
inline int overlap_lanes_for(int rw) { return (rw + PX - 1) / PX; }

hipError_t launch_apply(const float* src, const float* gain, const float* offset, float* out, int height, int width,
                        long long stride, hipStream_t stream);

// Block statistics for gain-blk-offset (kernel_model.py:216-229), per band.
// One plane of a BATCHED statistics launch (NormArgs::planes, device memory): plane p of the launch = (job, band)
struct NormPlane {
    const float* src;
    const float* ref;
    long long stride;
    int height, width;
};
struct NormArgs {
    const NormPlane* planes = nullptr;  // batched launch: n_bands entries (device), else NULL -- the planes are then src/ref + band * band_stride
    const float* src;
    const float* ref;
    int height, width;
    long long stride, band_stride;
    int n_bands;
    int src_nd_mode, ref_nd_mode;
    float src_nodata, ref_nodata;
    // batched launch: x-extent of the streaming pass's grid = the largest norm_pass_waves() over the planes (a plane with fewer
    // PIXELS than the largest one can still have more 1 KB chunks: width 1025 has 5 per row, width 1024 has 4); 0 = this shape's
    int grid_waves = 0;
};
// waves per plane of the streaming pass (a function of the plane's shape only)
int norm_pass_waves(int height, int width);
// workspace: norm_workspace_bytes() of device memory, laid out by norm_layout() (hk_layout.h); norm_out: n_bands x 2 float64 on device.
size_t norm_workspace_bytes(int n_bands, int height, int width);
// batched: a.planes set, a.n_bands planes, a.height x a.width = the LARGEST plane (sizes the workspace and the grid)
hipError_t launch_block_norm(const NormArgs& a, void* workspace, double* norm_out, hipStream_t stream);
// The same statistics for a block whose rows are spread over several ranks: six phases on this rank's slab, the caller
// all-reduces (SUM) the float64 exchange buffer (norm_split_exchange_doubles() values, device) between them.
size_t norm_split_exchange_doubles(int n_bands);
hipError_t launch_block_norm_split(const NormArgs& a, void* workspace, double* xchg, int phase,
                                   double* norm_out, hipStream_t stream);

// Masked comparison sums of homonim/compare.py:243-255 (hk_compare.hip), per band:
// sums_out[band * 7 + k] = [sum s, sum r, sum s^2, sum r^2, sum s*r, sum (r - s)^2, count] over jointly valid pixels.
struct CompareArgs {
    const float* src;
    const float* ref;
    int height, width;
    long long src_stride, ref_stride;            // elements between rows
    long long src_band_stride, ref_band_stride;  // elements between planes
    int n_bands;
    int src_nd_mode, ref_nd_mode;
    float src_nodata, ref_nodata;
    int vec_ok;                                  // set by the launcher: 16-byte row loads are legal
};
size_t compare_workspace_bytes(int n_bands);
hipError_t launch_compare_sums(const CompareArgs& a, void* workspace, double* sums_out, hipStream_t stream);

// Masked per-band statistics of a parameter image, homonim/stats.py:217-229 (hk_param_stats.hip), over the pixels valid under
// (nd_mode, nodata): stats_out[band * PARAM_STATS_N + k] =
//     [min, max, sum x, sum x^2, N, N(x < thresh), col_min, row_min, col_max, row_max]
// with x as float64; the last four are the bounding box of the valid pixels.  A band without a valid pixel gives
// [+inf, -inf, 0, 0, 0, 0, width, height, -1, -1].
constexpr int PARAM_STATS_N = 10;
struct ParamStatsArgs {
    const float* planes;
    int height, width;
    long long stride;       // elements between rows
    long long band_stride;  // elements between planes
    int n_bands;
    int nd_mode;
    float nodata;
    double thresh;
    int vec_ok;             // set by the launcher: 16-byte row loads are legal
};
size_t param_stats_workspace_bytes(int n_bands);
hipError_t launch_param_stats(const ParamStatsArgs& a, void* workspace, double* stats_out, hipStream_t stream);

// The raster that the overview and the DEFLATE launchers read: n_bands planes of height x width samples, strides in elements.
struct BandPlanes {
    const void* src;
    int n_bands, height, width;
    long long stride, band_stride;
};

// Average overviews (hk_overview.hip; homonim/fuse.py:152-165): level m = 1..n_levels of shape (ceil(height / 2^m),
// ceil(width / 2^m)), each the clipped 2 x 2 mean of the valid pixels of the level before it, all bands, OVERVIEW_PASS_LEVELS
// levels per launch.  dtype = hk_dtype; strides in elements; out[m - 1] / out_stride / out_band_stride describe level m.
constexpr int OVERVIEW_PASS_LEVELS = 6;
struct OverviewLevels {
    BandPlanes planes;
    int nd_mode;
    double nodata;
    int n_levels;  // any number: the launcher slices them into passes
    void* const* out;
    const long long* out_stride;
    const long long* out_band_stride;
    // the masked build (nullable `valid`: validity under nd_mode / nodata): a uint8 validity plane of the raster, 255 / 0, shared by
    // all bands -- nd_mode / nodata are not read then -- and one validity plane per level out; strides in bytes
    const unsigned char* valid = nullptr;
    long long valid_stride = 0;
    unsigned char* const* out_valid = nullptr;
    const long long* out_valid_stride = nullptr;
};
struct OverviewValid {  // the validity planes of one masked launch, beside its OverviewArgs
    const unsigned char* src;
    long long stride;
    unsigned char* out[OVERVIEW_PASS_LEVELS];
    long long out_stride[OVERVIEW_PASS_LEVELS];
    int vec_ok, out_vec_ok;  // set by the launcher: 16-byte loads of `src` / 8-byte level-1 stores are legal
};
struct OverviewArgs {
    const void* src;
    int height, width;
    long long stride, band_stride;
    int nd_mode;
    int n_levels;  // of this launch: 1..OVERVIEW_PASS_LEVELS
    double nodata;
    void* out[OVERVIEW_PASS_LEVELS];
    long long out_stride[OVERVIEW_PASS_LEVELS], out_band_stride[OVERVIEW_PASS_LEVELS];
    int vec_ok, out_vec_ok;  // set by the launcher: 16-byte row loads / 8-byte level-1 stores are legal
};
hipError_t launch_overviews(int dtype, const OverviewLevels& r, hipStream_t stream);

// DEFLATE streams of the tiles of a tiled GeoTIFF (hk_deflate.hip, which states the stream format): the raster's tiles of
// `tile` x `tile` samples of `esize` bytes, edge tiles zero-padded, in the order band, tile row, tile column; one zlib stream per
// tile into `out` at tile_offsets[t] (even), tile_sizes[t] bytes long; tile_offsets[n_tiles] = the bytes used.  Strides in
// elements.  `work`: deflate_workspace_bytes(number of chunks) of device memory; everything is queued on `stream`.
struct DeflateTiles {
    BandPlanes planes;
    int esize, tile;
    unsigned char* out;
    long long* tile_offsets;
    long long* tile_sizes;
};
struct DeflateArgs {
    const void* src;
    int es, height, width;
    long long stride, band_stride;
    int tile, across, down;   // tile size in samples, tiles per tile row, tile rows per band
    int tile_bytes, cpt;      // raw bytes and chunks per tile
    int vec_ok;               // set by the launcher: 16-byte row loads are legal
    unsigned char* slots;     // one slot per chunk
    unsigned* sizes;          // bytes of every chunk's block(s)
    unsigned* adler;          // per chunk: (sum of bytes mod 65521) | (weighted sum mod 65521) << 16
};
size_t deflate_workspace_bytes(long long n_chunks);
hipError_t launch_deflate_tiles(int predictor, const DeflateTiles& r, void* work, hipStream_t stream);
// the chunk kernel of predictors 2 and 3 (hk_deflate_pred.hip), launched by launch_deflate_tiles in place of deflate_chunk_kernel
hipError_t launch_deflate_pred_chunks(const DeflateArgs& a, int predictor, long long n_chunks, hipStream_t stream);

// The DEFLATE blocks (tiles or strips) of a GeoTIFF image inflated into a (spp, height, width) raster (hk_inflate.hip, which states
// the contract): block b's zlib stream is the sizes[b] bytes at streams + offsets[b]; blocks are ordered plane (separate only),
// block row, block column.  `work`: n_blocks slots of `slot` bytes (the raw size of a full block rounded up to 16; 16-byte
// aligned); status[b]: 0 or the HK_INFLATE_* code of a block that was refused and left out of the raster.  Strides in elements.
// All pointers are device memory; everything is queued on `stream`.
struct InflateArgs {
    const void* streams;
    const long long* offsets;
    const long long* sizes;
    unsigned char* work;
    int* status;
    void* out;
    long long stride, band_stride, slot;
    int es, height, width, bw, bh;   // sample bytes; the image; the block (a strip: bw = width)
    int tiled, separate, predictor;  // as hk_inflate_layout
    int cspp;                        // samples of a pixel in one block: spp of a pixel-interleaved image, else 1
    int across, down;                // blocks per block row, block rows
    int vec_ok;                      // set by the launcher: rows may move as 16-byte groups
};
hipError_t launch_inflate_image(InflateArgs a, long long n_blocks, hipStream_t stream);
// its second stage alone: the slots of the blocks with status 0 to the raster (untile_kernel<ES>; predictor 3: untile_fp_kernel<ES>)
hipError_t launch_untile(InflateArgs a, long long n_blocks, hipStream_t stream);
// The same for LZW blocks, TIFF compression 5 (hk_lzw.hip): status[b] is 0 or an HK_LZW_* code.
hipError_t launch_lzw_image(InflateArgs a, long long n_blocks, hipStream_t stream);
// ... and decoded on the calling thread (hk_lzw_host.hip: the host build of hk_lzw_core.h): every pointer is host memory,
// `work` is ONE slot, `status` may be NULL.  -> the first refused block (its status in *first_status), or -1.
long long lzw_image_host(const InflateArgs& a, long long n_blocks, int* first_status);

// the synthetic source / reference pair of the benchmark and the self-checks (hk_kernels.hip synth_kernel states the variants)
struct SynthFill {
    float* src;
    float* ref;
    int n_bands, height, width;
    long long stride, band_stride;
    unsigned long long seed;
    int nodata_variant;
};
hipError_t launch_synth_fill(const SynthFill& r, hipStream_t stream);

// Typed IO (hk_convert.hip).  dtype codes = hk_dtype of include/homonim_hk.h: 0 f32, 1 u8, 2 u16, 3 i16, 4 u32, 5 i32, 6 f64.
// One plane between `dtype` and float32: cast_in reads `in` as dtype and writes float32, cast_out reads float32 and writes dtype
// (NaN -> nodata when has_nodata, which cast_in does not read).  Strides in elements of each side's own type.
struct CastPlane {
    const void* in;
    long long in_stride;
    void* out;
    long long out_stride;
    int height, width;
    int has_nodata = 0;
    double nodata = 0.;
    unsigned char* valid = nullptr;  // launch_cast_out_valid: the validity plane (255 / 0), rows valid_stride bytes apart,
    long long valid_stride = 0;      // base and stride multiples of PX
};
hipError_t launch_cast_in(int dtype, const CastPlane& r, hipStream_t stream);
hipError_t launch_cast_out(int dtype, const CastPlane& r, hipStream_t stream);
// cast_out and, from the same read of the float32 plane, `valid` = 255 where it is not NaN, else 0 (every dtype, float32 included)
hipError_t launch_cast_out_valid(int dtype, const CastPlane& r, hipStream_t stream);
inline int dtype_size(int dtype) { const int sz[7] = {4, 1, 2, 2, 4, 4, 8}; return dtype >= 0 && dtype < 7 ? sz[dtype] : 0; }

// Resident rasters (hk_convert.hip).  The kernels' own argument structs carry typed pointers, so that the compiler knows their
// address space; the launchers take the untyped forms below.  Strides in elements of each side's own type.
template <typename T>
struct FillPlanes {
    T* __restrict__ out;
    long long stride, band_stride;
    int n_bands, height, width;
    T value;
};
template <typename T>
struct BoundlessWindow {
    const T* __restrict__ in;   // pixel (0, 0) of band 0 of the raster
    T* __restrict__ out_t;      // the window in the raster's own type (numeric nodata), or
    float* __restrict__ out_f;  // the window as float32 (no nodata value, or NaN): exactly one of the two is set
    long long in_stride, in_band_stride, out_stride, out_band_stride;
    int n_bands, height, width;                      // the raster
    int row_off, col_off, out_height, out_width;     // the window in raster coordinates: may hang over the raster or miss it
    T fill;
};
// `value` in every one of `width` samples of `height` rows of `n_bands` planes of dtype; the row padding is not written
struct PlaneFill {
    void* out;
    long long stride, band_stride;
    int n_bands, height, width;
    double value;
};
hipError_t launch_fill_planes(int dtype, const PlaneFill& r, hipStream_t stream);
// RasterFuse._read_boundless of all bands: the window (row_off, col_off, out_height, out_width) of a raster of dtype.  to_float:
// `out` is float32, the plain value conversion inside the raster and NaN outside; else `out` is of dtype with `fill` outside.
struct WindowGather {
    const void* in;
    long long in_stride, in_band_stride;
    int n_bands, height, width;
    int row_off, col_off, out_height, out_width;
    bool to_float;
    double fill;
    void* out;
    long long out_stride, out_band_stride;
};
hipError_t launch_boundless_window(int dtype, const WindowGather& r, hipStream_t stream);

// The per-dataset mask of a GeoTIFF applied to its bands (hk_dataset_mask.hip; homonim/raster_array.py:161-197): float32 planes
// `out` = valid ? (float)planes : NaN (0x7FC00000), the same validity for every band.  kind 0 (BITS): `mask` are packed rows of
// bits, most significant first, 1 = valid, mask_stride BYTES apart; kind 1 (ALPHA): a plane of the bands' sample type (uint8 /
// uint16 only), valid where it is not 0, mask_stride ELEMENTS apart.  dtype = hk_dtype; the other strides in elements.
struct DatasetMask {
    BandPlanes planes;
    const void* mask;
    int kind;
    long long mask_stride;
    float* out;
    long long out_stride, out_band_stride;
};
hipError_t launch_dataset_mask(int dtype, const DatasetMask& a, hipStream_t stream);

// mask_partial on a shared grid (hk_mask.hip): full-coverage mask from valid(in) & params, eroded by (kh+2) x (kw+2);
// writes masked parameters and/or the corrected block and/or the uint8 mask.  rowcnt_ws: height x stride uint16.
constexpr int ND_COVERAGE = 3;  // PartialMask::nd_mode: `in` is a coverage fraction, valid where it is >= 1 (nodata unused)
struct PartialMask {
    const float* in;
    int nd_mode;
    float nodata = 0.f;
    const float* params;  // n_bands planes band_stride apart, gain and offset first
    int n_bands;
    long long band_stride;
    const float* src = nullptr;  // read for corr_out only
    int height, width;
    long long stride;            // of every plane, the workspace included
    int kh, kw;
    // what to write, each or NULL: the masked parameters (n_bands planes), gain * src + offset under the mask, the mask as bytes
    float* params_out = nullptr;
    float* corr_out = nullptr;
    unsigned char* mask_out = nullptr;
};
hipError_t launch_partial_mask(const PartialMask& r, unsigned short* rowcnt_ws, hipStream_t stream);

// In-painting of the offset band (hk_inpaint.hip; GDALFillNodata restated): sources are pixels with r2 > thresh and
// gain > 0 (flag 1), flag 0 pixels are targets and are filled IN PLACE (a filled pixel never acts as a source: sources are read
// where the flag is 1 only), any other flag value is neither.
struct InpaintArgs {
    float* offset;     // the plane, filled in place
    long long stride;  // elements between rows: a multiple of 4 (the flag plane's and the table's rows move as quads)
    int height, width;
    // the source flags: either ready -- written by the fit kernel (FitArgs::flag; 1 byte per pixel, row stride `stride`), into
    // inpaint_flag_plane() of this workspace or anywhere else -- or NULL: made here from gain / r2 / thresh
    const unsigned char* flag_ready = nullptr;
    const float* gain = nullptr;
    const float* r2 = nullptr;
    float thresh = 0.f;
    unsigned long long n_targets = 0;  // failing pixels if the caller knows (0 = unknown): picks the order in which a tile's targets are searched
    bool packed_search = true;         // false (test aid only): the packed search is left out and the general one takes every target
};
// The workspace: inpaint_workspace_bytes() of device memory whose base is 16-byte aligned (hipErrorInvalidValue otherwise, nothing
// queued).  hk_layout.h inpaint_layout() states its pieces; inpaint_flag_plane() is the one a fit may write before the launch.
size_t inpaint_workspace_bytes(int height, long long stride);
unsigned char* inpaint_flag_plane(void* workspace, int height, long long stride);
hipError_t launch_inpaint_offsets(const InpaintArgs& a, void* workspace, hipStream_t stream);

// What every re-sampling launch carries, whatever maps a destination pixel to the source (hk_resample.hip, hk_warp.hip): hk_api.hip
// fills one per entry point, the kernels' argument structs embed it.  Strides in elements.
struct ResamplePlanes {
    const float* src;
    float* dst;
    long long src_stride, src_band_stride, dst_stride, dst_band_stride;
    int sh, sw, dh, dw, n_bands;
    int nd_mode;
    float nodata;
    float dst_fill;  // value of destination pixels that receive nothing
};
// kx, ky = source pixels per destination pixel.  An axis is down-sampled: bilinear / cubic_spline leave their 2 / 4-tap kernels for
// GWKResample, whose support scales with the step (cubic and lanczos always run it)
inline bool resample_stretched(double kx, double ky) { return kx > 1.0 + 1e-9 || ky > 1.0 + 1e-9; }

// Re-sampling between same-CRS axis-aligned grids (hk_resample.hip): src_col = kx * dst_col + ox, src_row = ky * dst_row + oy.
// mode = rasterio.enums.Resampling value (0..6, 8..14).
hipError_t launch_resample(int mode, const ResamplePlanes& p, double kx, double ox, double ky, double oy, hipStream_t stream);
constexpr int RS_NEAREST = 0, RS_AVERAGE = 5;  // the two modes that hk_api.hip asks for by itself
// `average` (mode 5) of ONE plane of sample type `dtype` (hk_dtype) read as it was uploaded: bit for bit launch_cast_in followed by
// launch_resample(5, ...) into `value` (pixels that receive nothing: `fill`) and, when `coverage` is not NULL, launch_valid_plane
// followed by launch_resample(5, ...) without nodata and fill 0 into it -- the typed pixels are read once.  Both destination planes
// have row stride dst_stride.  The kernel of sample type T receives FootTypedArgs<T>; the launcher takes FootTypedArgs<void>.
template <typename T>
struct FootTypedArgs {
    const T* src;
    long long src_stride;
    int sh, sw;
    int nd_mode;
    float nodata;
    float* value;
    float* coverage;  // nullable
    long long dst_stride;
    int dh, dw;
    float fill;
    double kx, ox, ky, oy;
};
hipError_t launch_footprint_typed(int dtype, const FootTypedArgs<void>& r, hipStream_t stream);

// Re-sampling between grids of two CRSs (hk_warp.hip): the continuous source pixel coordinates of the destination positions
// (row + off_row, col + off_col) of an h x w lattice, and launch_resample's modes 0..4 on them (kx, ky: the mean step, which picks
// and scales the stretched kernels).  `why` receives the reason when hipErrorInvalidValue is returned.
struct WarpLattice {
    double* x;
    double* y;
    long long stride;
    int h, w;
    double off_row, off_col;
};
hipError_t launch_warp_coords(const hk_warp_desc* desc, const WarpLattice& l, hipStream_t stream, const char** why);
hipError_t launch_warp_resample(int mode, const hk_warp_desc* desc, const ResamplePlanes& p, double kx, double ky,
                                hipStream_t stream, const char** why);
// The same for rotated / sheared grids, in one CRS or across two (hk_affine_warp_desc): full affines at both ends.
hipError_t launch_warp_coords(const hk_affine_warp_desc* desc, const WarpLattice& l, hipStream_t stream, const char** why);
hipError_t launch_warp_resample(int mode, const hk_affine_warp_desc* desc, const ResamplePlanes& p, double kx, double ky,
                                hipStream_t stream, const char** why);

size_t upsample_apply_workspace_bytes(int height);
// RefSpaceModel.apply fused with the up-sampling of its parameters (hk_resample.hip): out = gain * src + offset on the height x
// width source grid, gain / offset bilinear (mode 1) or cubic_spline (3) values of the coarse ph x pw planes under launch_resample's
// mapping, masked by `keep` where given, else by valid(src).  These are UpApplyArgs' fields, which the kernel receives, and the
// row axis (ky, oy) of the table that the launcher makes in `workspace`.
struct UpsampleApply {
    const float* src;
    long long src_stride;
    int nd_mode;
    float nodata;
    const float* gain;  // coarse parameter planes, NaN = nodata
    const float* offset;
    long long par_stride;
    int ph, pw;
    const float* keep = nullptr;  // full-resolution 0/1 plane (mask_partial)
    long long keep_stride = 0;
    float* out;
    long long out_stride;
    int height, width;
    double kx, ox, ky, oy;
};
hipError_t launch_upsample_apply(int mode, const UpsampleApply& r, void* workspace, hipStream_t stream);
// ... with the parameters already on the source grid: gain, offset and `keep` share par_stride
struct ApplySpace {
    const float* src;
    long long src_stride;
    int nd_mode;
    float nodata;
    const float* gain;
    const float* offset;
    long long par_stride;
    const float* keep = nullptr;
    float* out;
    long long out_stride;
    int height, width;
};
hipError_t launch_apply_space(const ApplySpace& r, hipStream_t stream);
// valid(in) as a float32 0/1 plane
struct ValidPlane {
    const float* in;
    long long in_stride;
    int nd_mode;
    float nodata;
    float* out;  // 1.f where `in` is valid, else 0.f
    long long out_stride;
    int height, width;
};
hipError_t launch_valid_plane(const ValidPlane& r, hipStream_t stream);

// flat 2-read 1-write float4 stream (measurement aid: what the HBM gives the fused kernel's byte mix without its stencil)
hipError_t launch_stream_probe(const void* a, const void* b, void* out, size_t n_bytes, hipStream_t stream);

// sum of the bit patterns of a height x width window of a float32 plane, modulo 2^64, ADDED to *out_dev (test / bench aid)
hipError_t launch_checksum(const float* plane, long long stride, int height, int width, unsigned long long* out_dev, hipStream_t stream);

// returns 0 on pass; writes a diagnostic code otherwise
hipError_t launch_selftest(int* result_dev, hipStream_t stream);

}  // namespace hk
