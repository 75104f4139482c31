/*
 * homonim_hk.h -- C ABI of the MI355X-native homonim kernel-model hot path (libhomonim_hk.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Every entry point names the
 * reference interface it replaces (paths relative to the reference repo leftfield-geospatial/homonim v0.4.3).
 * The reference has no FFI of its own (it is pure Python on top of OpenCV/GDAL wheels); the binding a maintainer
 * would add is a ctypes stub inside homonim/kernel_model.py -- shown in INTEGRATION.md and implemented in
 * homonim_amd/_hk.py.
 *
 * Conventions
 *   - All functions return 0 on success, a negative hk_status otherwise; hk_last_error() gives the text for the
 *     calling thread.  Nothing aborts the process.
 *   - Rasters are float32, row-major, one band per 2-D plane; `stride` is in ELEMENTS between rows.
 *   - nodata is passed as (mode, value): HK_NODATA_NONE = RasterArray.nodata is None (all pixels valid),
 *     HK_NODATA_NAN = nodata is NaN, HK_NODATA_VALUE = numeric nodata, compared with utils.nan_equals semantics
 *     (homonim/utils.py:54-56; homonim/raster_array.py:298-308).
 *   - kernel_shape is (kh, kw) = (rows, cols), both odd (homonim/utils.py:104-133).
 *   - Thread safety: any number of host threads may call into one hk_ctx concurrently (the reference calls
 *     fit/apply from a ThreadPoolExecutor on ONE shared model, homonim/fuse.py:396-401); each call checks a
 *     stream + staging slot out of the context's pool.
 */
#ifndef HOMONIM_HK_H
#define HOMONIM_HK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hk_ctx hk_ctx;
typedef struct hk_event hk_event;   /* a point in a context stream (hk_event_*, bottom of this header) */

typedef enum {
    HK_OK = 0,
    HK_ERR_ARG = -1,       /* bad argument (shape, kernel, null pointer ...) -> Python ValueError */
    HK_ERR_HIP = -2,       /* HIP runtime error -> Python RuntimeError */
    HK_ERR_NODEVICE = -3,  /* no usable GPU */
    HK_ERR_UNSUPPORTED = -4,
    HK_ERR_NOMEM = -5,
    HK_ERR_ALREADY = -6    /* hk_host_register: the range is page-locked already (nothing was changed; do not unregister it) */
} hk_status;

/* homonim/enums.py:22-41 (Model) */
typedef enum { HK_MODEL_GAIN = 0, HK_MODEL_GAIN_BLK_OFFSET = 1, HK_MODEL_GAIN_OFFSET = 2 } hk_model;

typedef enum { HK_NODATA_NONE = 0, HK_NODATA_NAN = 1, HK_NODATA_VALUE = 2 } hk_nodata_mode;

/*
 * Everything KernelModel.__init__ / create_config fix for the hot path (homonim/kernel_model.py:40-81,98-136)
 * plus the per-call nodata of the two RasterArrays.
 */
typedef struct {
    int32_t model;          /* hk_model */
    int32_t kh, kw;         /* kernel_shape (rows, cols), odd */
    int32_t find_r2;        /* KernelModel.find_r2: emit the R2 band (kernel_model.py:267-272,353-359) */
    int32_t has_r2_thresh;  /* r2_inpaint_thresh is not None (gain-offset only; kernel_model.py:325,361) */
    float r2_thresh;        /* r2_inpaint_thresh */
    int32_t src_nodata_mode;
    float src_nodata;
    int32_t ref_nodata_mode;
    float ref_nodata;
} hk_fit_desc;

/* ------------------------------------------------------------------------------------------------------------------
 * library / context
 */
/* Version of this header's struct layouts and prototypes.  A consumer built against one header and loading a library of
 * another must not call further: structs grow at their end between versions (hk_out_window: 32 -> 40 bytes in version 3) and
 * carry no size field; version 5 added entry points (hk_device_pci_bus_id; hk_debug_staging_counters in the devtools header); version 6: a raw
 * r2-mask failure counter is always a count (HK_COUNT_RETRY is never set any more), and a device-resident job that carries `scratch`
 * always gets the in-painting's inputs left there; version 7 added entry points (hk_param_stats, hk_param_stats_dev); version 8
 * added entry points (hk_overview_count, hk_overviews, hk_overviews_dev); version 9 added hk_crs_desc / hk_warp_desc and entry
 * points (hk_warp_coords, hk_warp_coords_dev, hk_reproject_crs, hk_reproject_crs_dev, hk_reproject_dev); version 10 added
 * hk_affine_warp_desc and entry points (hk_warp_coords_affine, hk_warp_coords_affine_dev, hk_reproject_affine,
 * hk_reproject_affine_dev); version 11 added hk_srcspace_desc and the entry point hk_srcspace_fit_apply; version 12 added entry
 * points (hk_deflate_bound, hk_deflate_tiles, hk_deflate_tiles_dev).  The inflate entry points (hk_inflate_bound,
 * hk_inflate_image, hk_inflate_image_dev, with the new struct hk_inflate_layout) were added WITHOUT a new version: no existing
 * layout or prototype changed, so a version-12 consumer runs unchanged against either library; a consumer that wants them looks
 * them up by symbol (dlsym) and does without where they are absent.  hk_deflate_tiles_pred and hk_deflate_tiles_pred_dev were
 * added the same way, and so were hk_dataset_mask and hk_dataset_mask_dev (plain scalar arguments, no struct), and the forms that
 * carry validity planes: hk_fit_apply_block_valid, hk_refspace_fit_apply_valid, hk_srcspace_fit_apply_valid, hk_overviews_valid and
 * hk_overviews_valid_dev (the structs they take are those of the entries they extend).  The device-resident two-grid entries
 * (hk_refspace_fit_apply_dev, hk_srcspace_fit_apply_dev, hk_refspace_dev_scratch_bytes, hk_srcspace_dev_scratch_bytes, with the new
 * struct hk_two_grid_job) were added the same way, and so were the entries of the resident rasters of RasterFuse.process
 * (hk_fill_planes_dev, hk_boundless_window_dev, hk_dev_mem_info: plain scalar arguments, no struct).
 * hk_abi_version() returns the library's HK_ABI_VERSION; compare it with the header's at load time. */
#define HK_ABI_VERSION 12
int hk_abi_version(void);
const char* hk_backend_name(void);            /* "hip-gfx950" */
const char* hk_last_error(void);              /* thread-local text of the last failure */
int hk_device_count(int* count);
/* PCI bus address of HIP device `device_id` as sysfs spells it ("0000:c1:00.0"; `len` >= 13), so that a rank can look up its
 * GPU's NUMA node (/sys/bus/pci/devices/<address>/numa_node) and run its host threads -- the staging copies, the pinned
 * allocations -- on that node's cores (homonim_amd/topology.py).  The reference's "devices" are the host's own cores
 * (homonim/fuse.py:396-401: a ThreadPoolExecutor); there is nothing to place. */
int hk_device_pci_bus_id(int device_id, char* out, int len);
/* One context per GPU: owns `n_streams` HIP streams, each with a pinned-host + device staging slot that grows on
 * demand.  Replaces nothing in the reference (its "device" is the host CPU); mirrors the thread pool of
 * homonim/fuse.py:396.
 * No process-wide side effects by default; the diagnostic switches (HK_FAULT_REPORT=1, HK_GUARD_ALLOC) are described in
 * homonim_hk_devtools.h.  Every entry point that selects the context's device also clears the calling thread's sticky HIP
 * "last error" (hipGetLastError), so that an error this library reported does not resurface in the caller's next launch. */
int hk_ctx_create(int device_id, int n_streams, hk_ctx** ctx);
int hk_ctx_destroy(hk_ctx* ctx);
int hk_ctx_sync(hk_ctx* ctx);                 /* hipDeviceSynchronize on the context's device */

/* ------------------------------------------------------------------------------------------------------------------
 * host-pointer entry points (numpy arrays in, numpy arrays out): H2D -> kernels -> D2H on one pooled stream.
 */

/* KernelModel._fit_block_norm (homonim/kernel_model.py:216-229): norm[0] = std(ref[mask]) / std(src[mask]),
 * norm[1] = percentile(ref[mask], 1) - percentile(src[mask], 1) * norm[0]; [0, 0] when no pixel is valid. */
int hk_block_norm(hk_ctx* ctx, const hk_fit_desc* desc, const float* src, int64_t src_stride, const float* ref,
                  int64_t ref_stride, int32_t height, int32_t width, double norm_out[2]);

/* RasterCompare.process / get_block_sums (homonim/compare.py:243-255) for one band of two rasters on the same grid:
 * sums_out = [ sum src, sum ref, sum src^2, sum ref^2, sum src*ref, sum (ref - src)^2, N ] over jointly valid pixels
 * (see hk_compare_sums_dev for the arithmetic). */
int hk_compare_sums(hk_ctx* ctx, const float* src, int64_t src_stride, int32_t src_nodata_mode, float src_nodata,
                    const float* ref, int64_t ref_stride, int32_t ref_nodata_mode, float ref_nodata, int32_t height,
                    int32_t width, double sums_out[7]);

/* ParamStats.stats / get_block_sums (homonim/stats.py:217-229) and the data window of stats.py:135-173 for one band (or one
 * strip of rows of a band) of a parameter image in host memory:
 * stats_out = [ min, max, sum x, sum x^2, N, N(x < thresh), col_min, row_min, col_max, row_max ] over the valid pixels
 * (see hk_param_stats_dev for the arithmetic and the empty band).  Strips combine exactly: min of mins, max of maxes, sums of
 * sums and counts, union of boxes (row indices are relative to the strip). */
int hk_param_stats(hk_ctx* ctx, const float* plane, int64_t stride, int32_t nodata_mode, float nodata, double thresh,
                   int32_t height, int32_t width, double stats_out[10]);

/* The number of internal overviews RasterFuse.build_overviews gives a raster of this shape (homonim/fuse.py:152-165):
 * n = min(8, int(min(log2(height), log2(width))) - 8), never below 0; the factors are 2^1 .. 2^n, so that the coarsest level
 * keeps at least 256 pixels on the shorter side.  Plain host arithmetic (no device needed). */
int hk_overview_count(int32_t height, int32_t width, int32_t* n);

/* Average overviews of an n_bands x height x width raster of sample type `dtype` (hk_dtype, below) in host memory (plane b at
 * planes + b * band_stride, `stride` elements between rows): level m = 1..n_levels, of shape (ceil(height / 2^m),
 * ceil(width / 2^m)), into out[m - 1] (host; out_stride[m - 1] elements between rows, out_band_stride[m - 1] between planes).
 * See hk_overviews_dev for the arithmetic.  The raster travels in strips of whole rows, each a multiple of 2^n_levels rows and at
 * most 64 MiB over all bands (HK_OVERVIEW_STRIP_KB lowers the bound, for tests): no cell of any level straddles two strips, so
 * neither the strip size nor the layout of the arrays changes a bit of the result. */
int hk_overviews(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                 int64_t band_stride, int32_t nodata_mode, double nodata, int32_t n_levels, void* const out[],
                 const int64_t out_stride[], const int64_t out_band_stride[]);

/* hk_overviews under a per-dataset validity mask instead of a nodata value -- the overviews of a file that is written with an
 * internal mask (RasterArray.to_rio_dataset's write_mask, homonim/raster_array.py:493-500, and build_overviews on that dataset).
 * `valid`: height rows of one byte per pixel in host memory, valid_stride bytes apart, valid where not 0, one plane for all bands.
 * out_valid[m - 1] (host; out_valid_stride[m - 1] bytes between rows) receives level m's own validity, 255 / 0.  See
 * hk_overviews_valid_dev for the rule.  Strips as in hk_overviews, HK_OVERVIEW_STRIP_KB included. */
int hk_overviews_valid(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                       int64_t band_stride, const uint8_t* valid, int64_t valid_stride, int32_t n_levels, void* const out[],
                       const int64_t out_stride[], const int64_t out_band_stride[], uint8_t* const out_valid[],
                       const int64_t out_valid_stride[]);

/* The per-dataset mask of a GeoTIFF -- an internal 1-bit mask or an alpha band -- applied to its bands, as
 * RasterArray.from_rio_dataset reads such a file (homonim/raster_array.py:161-197): out[b][y][x] = valid(y, x) ?
 * (float)planes[b][y][x] : NaN (bit pattern 0x7FC00000), the same validity for every band; the conversion is the plain value
 * conversion of every other input (exact for 8/16-bit integers, round to nearest for 32-bit integers and float64; a valid float32
 * keeps its bits).  `planes`: n_bands x height x width samples of `dtype` (hk_dtype, below) in host memory, `stride` elements
 * between rows, band b at planes + b * height * stride; `out`: float32, out_stride elements between rows, band b at out + b *
 * height * out_stride.  mask_kind HK_MASK_BITS: `mask` are `height` rows of packed bits, the most significant bit of a byte first,
 * 1 = valid, mask_stride BYTES apart (>= ceil(width / 8); the pad bits of a row's last byte are not looked at); HK_MASK_ALPHA:
 * a plane of the SAME sample type as the bands, which must be HK_DTYPE_U8 or HK_DTYPE_U16, mask_stride ELEMENTS apart (>= width),
 * a pixel being valid where its alpha sample is not 0.  Nothing outside [row, row + width) of any plane and outside ceil(width / 8)
 * bytes of a mask row is read or written.  The raster travels in chunks of whole rows of at most 64 MiB on the device
 * (HK_STAGE_CHUNK_KB, read at every call, lowers the bound for tests); rows are independent, so the chunking cannot change a bit.  See hk_dataset_mask_dev.
 * HK_ERR_ARG, naming the argument: an unknown dtype or mask_kind, HK_MASK_ALPHA with another dtype, a NULL pointer, a size below
 * 1, stride or out_stride < width, mask_stride too small. */
enum { HK_MASK_BITS = 0, HK_MASK_ALPHA = 1 };
int hk_dataset_mask(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                    const void* mask, int32_t mask_kind, int64_t mask_stride, float* out, int64_t out_stride);

/* DEFLATE on the device: one zlib stream per tile of a tiled, band-separate GeoTIFF (homonim/fuse.py:124-149: tiled, compress =
 * deflate, interleave = band), in place of zlib.compress on a host thread.  A tile is `tile` x `tile` samples (`tile` a multiple of
 * 16 in 16..512), little-endian, edge tiles zero-padded; tiles are ordered band, tile row, tile column.  Every stream is: 78 9C; per
 * HK_DEFLATE_CHUNK raw bytes either one dynamic-Huffman block followed by an empty stored block, or one stored block (whenever the
 * former would not be smaller); a final empty fixed block (03 00); the Adler-32.  Matches are runs at two distances only, the sample
 * size and the tile's row length; the bytes are a function of the input alone.  Any inflater reads the streams; they are a few
 * percent larger than zlib level 6. */
#define HK_DEFLATE_CHUNK 16384
/* n_tiles = n_bands x ceil(height / tile) x ceil(width / tile); bytes = the capacity that always suffices: per tile
 * 2 + sum over its chunks (chunk + 5) + 6, rounded up to even.  Plain host arithmetic (no device needed). */
int hk_deflate_bound(int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int32_t tile, int64_t* n_tiles, int64_t* bytes);
/* The streams of a raster in host memory (plane b at planes + b * band_stride, `stride` elements between rows) into `out` (host,
 * out_capacity >= hk_deflate_bound's bytes): tile t's stream is the tile_sizes[t] bytes at out + tile_offsets[t]; offsets are even
 * (an odd stream is followed by one zero byte, as a TIFF writer pads it) and increasing, tile_offsets[n_tiles] = the bytes used.
 * The raster travels through the pinned staging ring in groups of whole tile rows of one band, at most 64 MiB of raw bytes each
 * (HK_DEFLATE_GROUP_KB lowers the bound, for tests), and only compressed bytes come back. */
int hk_deflate_tiles(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                     int64_t band_stride, int32_t tile, void* out, int64_t out_capacity, int64_t* tile_offsets /* n_tiles + 1 */,
                     int64_t* tile_sizes /* n_tiles */);
/* hk_deflate_tiles over the PREDICTED bytes of every tile (TIFF tag 317), for a file that carries the Predictor tag.  The predictor
 * runs over each zero-padded tile row of `tile` samples on its own.  1: none -- exactly the bytes of hk_deflate_tiles.  2 (integer
 * dtypes): p[i] = s[i] - s[i - 1] modulo 2^(8 x sample size), p[0] = s[0], samples little-endian; the step from the last pixel into the
 * padding is part of the row.  3 (HK_DTYPE_F32 / F64; libtiff's floating-point predictor): the row's bytes regrouped into planes of
 * `tile` bytes, most significant byte of every sample first, then differenced byte by byte modulo 256 over the whole row.  The stream
 * is the one described above with the predicted bytes in place of the raw ones (the Adler-32 too); the first match distance is the
 * sample size with predictors 1 and 2 and ONE with predictor 3.  hk_deflate_bound holds unchanged.  Predictor 2 with a float dtype,
 * 3 with an integer dtype and every other value: HK_ERR_ARG, before anything else is looked at.  Added to version 12 without a new
 * version, like the inflate entry points: look the symbol up where an older library may be loaded. */
int hk_deflate_tiles_pred(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                          int64_t stride, int64_t band_stride, int32_t tile, void* out, int64_t out_capacity,
                          int64_t* tile_offsets /* n_tiles + 1 */, int64_t* tile_sizes /* n_tiles */, int32_t predictor);

/* INFLATE on the device: the DEFLATE blocks (tiles or strips) of one GeoTIFF image, compression 8 or 32946, inflated and put in
 * their place in a (spp, height, width) raster, in place of zlib.decompress + the predictor + a slice copy per block on a host
 * thread.  A block's stream may be any legal zlib stream (stored, fixed and dynamic blocks, 15-bit codes, distances to 32768,
 * lengths to 258, overlapping copies) that inflates to exactly the block's raw size; bytes behind its Adler-32 are ignored.
 * Every block gets a status: 0, or why its stream was refused -- such a block is left out of the raster (the device call does not
 * write its pixels; the host call leaves them unspecified) and does not disturb the others.  Blocks are ordered plane (separate only), block row, block column, as TIFF
 * orders them.
 * The predictor (TIFF tag 317) is undone behind the decoder, row by block row.  2: s[i] = p[i] + s[i - 1] per sample of a pixel,
 * modulo 2^(8 x sample_bytes).  3 (sample_bytes 4 and 8 only; libtiff's floating-point predictor): the row's block_w x (separate ?
 * 1 : spp) x sample_bytes bytes are summed byte by byte modulo 256 at a distance of (separate ? 1 : spp) over the WHOLE row,
 * straight across the plane boundaries; the summed row is sample_bytes planes of block_w x (separate ? 1 : spp) bytes, the most
 * significant byte of every sample first, and the sample that is stored is little-endian.  The row is block_w wide in an edge
 * tile too.  (The field took 1 and 2 at first; 3 was admitted later without a new version: an older library refuses it.) */
typedef struct hk_inflate_layout {
    int32_t sample_bytes;      /* 1, 2, 4, 8; little-endian samples */
    int32_t spp, height, width;
    int32_t block_w, block_h;  /* tile size; strips: width, rows per strip */
    int32_t tiled;             /* 1: every block holds block_h rows; 0: the last strip is short */
    int32_t separate;          /* 1: one plane per block, blocks ordered plane, block row, block column; 0: pixel-interleaved */
    int32_t predictor;         /* 1 none, 2 horizontal differencing, 3 floating point (sample_bytes 4 and 8 only) */
} hk_inflate_layout;
enum {
    HK_INFLATE_OK = 0,
    HK_INFLATE_TRUNCATED = 1,   /* a bit past the stream's end was needed (an empty or missing stream too) */
    HK_INFLATE_BAD_HEADER = 2,  /* zlib header: method not 8, window above 32 KiB, FCHECK, or a preset dictionary */
    HK_INFLATE_BAD_BLOCK = 3,   /* block type 3 */
    HK_INFLATE_BAD_STORED = 4,  /* stored block: LEN != ~NLEN */
    HK_INFLATE_BAD_CODE = 5,    /* dynamic header: too many symbols, an over-subscribed or incomplete code, a bad repeat, no end-of-block code */
    HK_INFLATE_BAD_SYMBOL = 6,  /* literal/length symbol 286 / 287, distance symbol 30 / 31, or bits that are no code of the set */
    HK_INFLATE_FAR = 7,         /* a distance larger than the bytes produced so far */
    HK_INFLATE_OVERRUN = 8,     /* the stream holds more than the block's raw size */
    HK_INFLATE_SHORT = 9,       /* the stream ends before the block's raw size */
    HK_INFLATE_ADLER = 10       /* the Adler-32 of the bytes is not the stream's */
};
#define HK_INFLATE_MAX_BLOCK (1 << 30)   /* largest raw size of one block, bytes */
/* n_blocks = (separate ? spp : 1) x ceil(height / block_h) x ceil(width / block_w); raw_block_bytes = block_h x block_w x
 * (separate ? 1 : spp) x sample_bytes, the raw size of a full block; work_bytes = n_blocks x raw_block_bytes rounded up to 16: the
 * device scratch of hk_inflate_image_dev.  Plain host arithmetic (no device needed). */
int hk_inflate_bound(const hk_inflate_layout* layout, int64_t* n_blocks, int64_t* raw_block_bytes, int64_t* work_bytes);
/* The image of `layout` from block streams in host memory -- block b's stream is the sizes[b] bytes at streams + offsets[b] --
 * into `out` (host; plane c at out + c * band_stride, `stride` elements between rows; elements of sample_bytes).  The compressed
 * bytes go up and the raster comes down through the pinned staging ring, in groups of whole block rows of at most 64 MiB of raw
 * bytes (HK_INFLATE_GROUP_KB lowers the bound, for tests).  `status`: n_blocks values or NULL.  If any block was refused the call
 * returns HK_ERR_ARG, hk_last_error() names the first such block and the reason, `status` is filled all the same and every other
 * block is in `out`. */
int hk_inflate_image(hk_ctx* ctx, const hk_inflate_layout* layout, const void* streams, const int64_t* offsets, const int64_t* sizes,
                     void* out, int64_t stride, int64_t band_stride, int32_t* status /* n_blocks or NULL */);

/* LZW on the device and on the host: the LZW blocks (tiles or strips) of one GeoTIFF image, compression 5, decoded and put in their
 * place like the DEFLATE ones above -- same layout struct, same hk_inflate_bound, same block order, slots and staging groups
 * (HK_INFLATE_GROUP_KB), same error convention.  A block's stream is TIFF 6.0 LZW: codes of 9 to 12 bits, most significant bit
 * first; 0..255 bytes, 256 Clear, 257 end of information, entries from 258; the width grows once the next free entry is
 * 2^width - 1 (libtiff's early change); a full table adds nothing more; the stream starts as if behind a Clear.  Decoding ends
 * with the block's raw size: a last string is cut and nothing behind it is looked at (a missing end code is fine).  Every block
 * gets a status, with the same meaning in all three calls.  Added to version 12 without a new version: look the symbols up. */
enum {
    HK_LZW_OK = 0,
    HK_LZW_TRUNCATED = 1,   /* a bit past the stream's end was needed (an empty or missing stream too) */
    HK_LZW_OLD_STYLE = 2,   /* the pre-6.0 bit order (libtiff's test: first byte 0, bit 0 of the second set): not decoded */
    HK_LZW_BAD_FIRST = 3,   /* the first code after a Clear is above 257 */
    HK_LZW_BAD_CODE = 4,    /* a code above the next free entry */
    HK_LZW_SHORT = 5        /* end of information before the block's raw size */
};
/* hk_inflate_image for LZW streams. */
int hk_lzw_image(hk_ctx* ctx, const hk_inflate_layout* layout, const void* streams, const int64_t* offsets, const int64_t* sizes,
                 void* out, int64_t stride, int64_t band_stride, int32_t* status /* n_blocks or NULL */);
/* The same image from the same arguments decoded on the calling thread: the decoder of the kernel compiled for the host, then crop,
 * de-interleaving and predictors 2 and 3 in plain C++.  No context, no device (like hk_inflate_bound); `out` aligned to its samples. */
int hk_lzw_image_host(const hk_inflate_layout* layout, const void* streams, const int64_t* offsets, const int64_t* sizes, void* out,
                      int64_t stride, int64_t band_stride, int32_t* status /* n_blocks or NULL */);

/* KernelModel.fit (homonim/kernel_model.py:411-440 -> _fit_gain :231-274, _fit_gain_blk_offset :276-303,
 * _fit_gain_offset :305-373, _r2_array :142-214).
 *   params_out : n_param_bands x height x width float32, band 0 gain, 1 offset, 2 R2 (iff n_param_bands == 3;
 *                must equal 3 exactly when find_r2 || (model == gain-offset && has_r2_thresh)), NaN outside mask.
 *   norm_in    : gain-blk-offset only: float64[2] block normalisation to use, or NULL to compute it (hk_block_norm).
 *   norm_out   : optional float64[2], receives the normalisation actually used.
 *   r2_fail_count : optional; gain-offset with has_r2_thresh: number of valid pixels failing
 *                (r2 > thresh) & (gain > 0) (kernel_model.py:363).  When it is 0 the reference's in-paint branch is
 *                the identity; when > 0 the offsets of those pixels have been in-painted from the passing ones and
 *                their gains recomputed on the device (kernel_model.py:364-371; restated GDALFillNodata, hk_inpaint.hip)
 *                before params_out is written.
 * Unlike the reference, src/ref are NOT modified (no in-place zero-fill, kernel_model.py:246-247,320-321). */
int hk_fit(hk_ctx* ctx, const hk_fit_desc* desc, const float* src, int64_t src_stride, const float* ref,
           int64_t ref_stride, int32_t height, int32_t width, const double* norm_in, float* params_out,
           int32_t n_param_bands, double* norm_out, uint64_t* r2_fail_count);

/* KernelModel.apply (homonim/kernel_model.py:442-463): out = params[0] * src + params[1] (two float32 roundings). */
int hk_apply(hk_ctx* ctx, const float* src, int64_t src_stride, const float* params /* 2 x H x W */,
             int32_t height, int32_t width, float* out);

/* fit + apply of RasterFuse._process_block (homonim/fuse.py:305-307) fused in one pass: window sums, solve, R2 test
 * and correction in a single kernel; parameters are materialised only if params_out != NULL. */
int hk_fit_apply(hk_ctx* ctx, const hk_fit_desc* desc, const float* src, int64_t src_stride, const float* ref,
                 int64_t ref_stride, int32_t height, int32_t width, const double* norm_in,
                 float* params_out /* nullable */, int32_t n_param_bands, float* corr_out, double* norm_out,
                 uint64_t* r2_fail_count);

/* RasterArray.reproject (homonim/raster_array.py:526-578 -> GDAL warp) between two grids of the SAME CRS that are north-up
 * and axis-aligned, as RefSpaceModel / SrcSpaceModel call it (homonim/kernel_model.py:397,480,491,497,520).
 *   mapping   : src_col = kx * dst_col + ox, src_row = ky * dst_row + oy on continuous pixel coordinates whose integers
 *               are pixel edges (kx, ky > 0);
 *   resampling: rasterio.enums.Resampling value -- 0 nearest, 1 bilinear, 3 cubic_spline (both up-sampling only),
 *               5 average;
 *   src       : n_bands x src_h x src_w float32 with the given nodata; dst: n_bands x dst_h x dst_w float32, pixels that
 *               receive nothing are set to dst_fill (the destination nodata; 0 when that is None). */
int hk_reproject(hk_ctx* ctx, const float* src, int32_t n_bands, int32_t src_height, int32_t src_width,
                 int32_t src_nodata_mode, float src_nodata, double kx, double ox, double ky, double oy, int32_t resampling,
                 float* dst, int32_t dst_height, int32_t dst_width, float dst_fill);

/* RasterArray.reproject (homonim/raster_array.py:526-578) between grids of DIFFERENT coordinate reference systems, and the
 * up-front warp of utils.same_orientation_crs (homonim/utils.py:190-209), which brings the processing-grid image of a
 * RasterPairReader into the other image's CRS (homonim/raster_pair.py:160-166).
 * A CRS is geographic (coordinates in degrees, longitude first) or Transverse Mercator on an ellipsoid (a, 1 / f; inv_f = 0: a
 * sphere); there are no datum shifts: the two CRSs of a warp share their ellipsoid (HK_ERR_UNSUPPORTED otherwise).  Transverse
 * Mercator is the Krueger series in n to n^6 (Karney 2011), float64 throughout: every destination pixel is transformed exactly
 * (GDAL's default warp interpolates the transformation within 0.125 pixel).  Geo-transforms are axis-aligned:
 * x = gt[0] + col * gt[1], y = gt[2] + row * gt[3] on continuous pixel coordinates whose integers are pixel edges. */
typedef enum { HK_CRS_GEOGRAPHIC = 0, HK_CRS_TMERC = 1 } hk_crs_kind;
typedef struct hk_crs_desc {
    int32_t kind;      /* hk_crs_kind */
    int32_t reserved;  /* 0 */
    double a, inv_f;   /* ellipsoid: semi-major axis (metres), inverse flattening */
    double lat0, lon0; /* Transverse Mercator: latitude of origin, central meridian (degrees); geographic: 0 */
    double k0;         /* scale factor on the central meridian */
    double fe, fn;     /* false easting / northing (metres) */
} hk_crs_desc;
typedef struct hk_warp_desc {
    hk_crs_desc src_crs, dst_crs;
    double src_gt[4], dst_gt[4];
} hk_warp_desc;
/* The continuous SOURCE pixel coordinates (column into x_out, row into y_out; float64, `stride` elements between rows) of the
 * destination positions (row + off_row, col + off_col), row < height, col < width: offsets 0.5 give the pixel centres, offsets 0
 * on a (dst_height + 1) x (dst_width + 1) lattice the pixel corners.  NaN where a position has no image in the source CRS
 * (|latitude| > 90 degrees, 90 degrees or more from a Transverse Mercator's central meridian).  These are, bit for bit, the
 * coordinates hk_reproject_crs* uses for the same descriptor at offsets 0.5.  Elements between a row's end and `stride` are not
 * written.  hk_warp_coords: host planes; hk_warp_coords_dev: device planes, asynchronous on pooled stream `stream`. */
int hk_warp_coords(hk_ctx* ctx, const hk_warp_desc* warp, double off_row, double off_col, int32_t height, int32_t width,
                   double* x_out, double* y_out, int64_t stride);
int hk_warp_coords_dev(hk_ctx* ctx, const hk_warp_desc* warp, double off_row, double off_col, int32_t height, int32_t width,
                       double* x_dev, double* y_dev, int64_t stride, int32_t stream);
/* hk_reproject across CRSs: per destination pixel the source coordinate comes from `warp` instead of an affine mapping, the
 * re-sampling arithmetic is hk_reproject's own.  resampling: 0 nearest, 1 bilinear, 2 cubic, 3 cubic_spline, 4 lanczos (the
 * footprint methods -- average, mode, max, min, med, q1, q3, sum, rms -- are HK_ERR_UNSUPPORTED across CRSs: the reference's
 * up-front warp is bilinear).  kx, ky (> 0): source pixels per destination pixel, the mean step along the destination's central
 * row / column; they pick the stretched (down-sampling) kernels and scale their support as hk_reproject's kx, ky do.  A pixel
 * whose coordinate is NaN or lies outside the source gets dst_fill.  All bands are re-sampled in one launch; a thread computes
 * its pixel's coordinate once.  hk_reproject_crs: host rasters, contiguous like hk_reproject's; hk_reproject_crs_dev: device
 * rasters (strides in elements), asynchronous on pooled stream `stream`. */
int hk_reproject_crs(hk_ctx* ctx, const hk_warp_desc* warp, const float* src, int32_t n_bands, int32_t src_height,
                     int32_t src_width, int32_t src_nodata_mode, float src_nodata, double kx, double ky, int32_t resampling,
                     float* dst, int32_t dst_height, int32_t dst_width, float dst_fill);
int hk_reproject_crs_dev(hk_ctx* ctx, const hk_warp_desc* warp, const float* src_dev, int32_t n_bands, int32_t src_height,
                         int32_t src_width, int64_t src_stride, int64_t src_band_stride, int32_t src_nodata_mode,
                         float src_nodata, double kx, double ky, int32_t resampling, float* dst_dev, int32_t dst_height,
                         int32_t dst_width, int64_t dst_stride, int64_t dst_band_stride, float dst_fill, int32_t stream);
/* Rotated and sheared grids: what utils.same_orientation_crs (homonim/utils.py:182-209) obtains from a bilinear WarpedVRT for
 * every image that is not north-up, and RasterArray.reproject between such grids.  The geo-transforms are full affines in Affine
 * order (a, b, c, d, e, f): x = a * col + b * row + c, y = d * col + e * row + f on continuous pixel coordinates whose integers
 * are pixel edges.  Per destination position, float64, in exactly this association:
 *   X = (c + col * a) + row * b, Y = (f + col * d) + row * e                      (destination geo-transform)
 *   (x, y) = (X, Y) when same_crs != 0; otherwise destination CRS -> (lon, lat) -> source CRS as for hk_warp_desc
 *   u = x - sc, v = y - sf, col_s = (u * se - v * sb) / det, row_s = (v * sa - u * sd) / det   (source geo-transform)
 * with det = sa * se - sb * sd formed once on the host.  same_crs != 0: the two grids share their CRS, whatever it is; src_crs
 * and dst_crs are ignored, so CRSs this library cannot define are served too.  Every pixel is transformed exactly (GDAL's
 * default warp interpolates the transformation within 0.125 pixel).  A non-finite coefficient or a zero determinant of either
 * geo-transform is HK_ERR_ARG.  These builds run on a two-dimensional thread tile: 32 x 8 destination pixels, a provisional
 * choice until tools/warp_timing.py has been run (HK_WARP_TILE=WxH with W * H = 256, read once, overrides it -- a measurement
 * aid, the results do not depend on it). */
typedef struct hk_affine_warp_desc {
    hk_crs_desc src_crs, dst_crs;
    int32_t same_crs;  /* non-zero: one CRS, src_crs / dst_crs are ignored */
    int32_t reserved;  /* 0 */
    double src_gt[6], dst_gt[6];
} hk_affine_warp_desc;
/* hk_warp_coords / hk_warp_coords_dev / hk_reproject_crs / hk_reproject_crs_dev for an hk_affine_warp_desc: the same arguments, the
 * same staging and the same errors (the footprint methods are HK_ERR_UNSUPPORTED here as well).  The coordinates are, bit for
 * bit, the ones the re-samplers use.  kx, ky: source pixels per destination pixel, the lengths of the destination's column and
 * row steps in source pixels. */
int hk_warp_coords_affine(hk_ctx* ctx, const hk_affine_warp_desc* warp, double off_row, double off_col, int32_t height,
                          int32_t width, double* x_out, double* y_out, int64_t stride);
int hk_warp_coords_affine_dev(hk_ctx* ctx, const hk_affine_warp_desc* warp, double off_row, double off_col, int32_t height,
                              int32_t width, double* x_dev, double* y_dev, int64_t stride, int32_t stream);
int hk_reproject_affine(hk_ctx* ctx, const hk_affine_warp_desc* warp, const float* src, int32_t n_bands, int32_t src_height,
                        int32_t src_width, int32_t src_nodata_mode, float src_nodata, double kx, double ky, int32_t resampling,
                        float* dst, int32_t dst_height, int32_t dst_width, float dst_fill);
int hk_reproject_affine_dev(hk_ctx* ctx, const hk_affine_warp_desc* warp, const float* src_dev, int32_t n_bands,
                            int32_t src_height, int32_t src_width, int64_t src_stride, int64_t src_band_stride,
                            int32_t src_nodata_mode, float src_nodata, double kx, double ky, int32_t resampling, float* dst_dev,
                            int32_t dst_height, int32_t dst_width, int64_t dst_stride, int64_t dst_band_stride, float dst_fill,
                            int32_t stream);
/* hk_reproject on device-resident rasters (strides in elements), asynchronous on pooled stream `stream`: the same kernels, the
 * same bits. */
int hk_reproject_dev(hk_ctx* ctx, const float* src_dev, int32_t n_bands, int32_t src_height, int32_t src_width,
                     int64_t src_stride, int64_t src_band_stride, int32_t src_nodata_mode, float src_nodata, double kx, double ox,
                     double ky, double oy, int32_t resampling, float* dst_dev, int32_t dst_height, int32_t dst_width,
                     int64_t dst_stride, int64_t dst_band_stride, float dst_fill, int32_t stream);

/* `mask_partial` on a shared grid: KernelModel._full_coverage_mask (homonim/kernel_model.py:375-409) -- the mask of
 * pixels that are valid in `in` (nodata as given) and have parameters, eroded by a (kh+2) x (kw+2) rectangle with a
 * zero border -- followed by what the reference does with it:
 *   RefSpaceModel.apply (:493-503): in = the source block, corr_out = gain * src + offset with parameters outside the
 *                                   mask set to NaN (pass src = in);
 *   SrcSpaceModel.fit   (:526-531): in = the reference block, params_out = all n_param_bands masked.
 * params: n_param_bands x H x W float32 (band 0 gain, 1 offset); params_out / corr_out / mask_out (uint8) nullable.
 * in_nodata_mode 3 = `in` is a coverage fraction (the mask re-projected with `average`): valid where in >= 1 (:399). */
int hk_partial_mask(hk_ctx* ctx, const float* in, int64_t in_stride, int32_t in_nodata_mode, float in_nodata,
                    const float* params, int32_t n_param_bands, const float* src, int64_t src_stride, int32_t height,
                    int32_t width, int32_t kh, int32_t kw, float* params_out, float* corr_out, uint8_t* mask_out);

/* Typed rasters either side of the path: integer / float64 inputs are converted to float32 on the device exactly as
 * RasterArray.from_rio_dataset reads them (homonim/raster_array.py:178-188), the corrected block is converted to the
 * output dtype as RasterArray._convert_array_dtype does for to_rio_dataset (homonim/raster_array.py:353-387: round
 * half-to-even, clip, masked pixels -> out_nodata).  PCIe then carries 1-2 B per pixel instead of 4. */
typedef enum { HK_DTYPE_F32 = 0, HK_DTYPE_U8 = 1, HK_DTYPE_U16 = 2, HK_DTYPE_I16 = 3, HK_DTYPE_U32 = 4, HK_DTYPE_I32 = 5,
               HK_DTYPE_F64 = 6 } hk_dtype;
typedef struct {
    int32_t src_dtype, ref_dtype;  /* hk_dtype of the src / ref host arrays */
    int32_t out_dtype;             /* hk_dtype of corr_out */
    int32_t out_has_nodata;        /* 0: masked pixels keep NaN (float outputs) / become 0 (integer outputs) */
    double out_nodata;
} hk_io_desc;
/* hk_fit_apply with typed src / ref / corr_out (strides in ELEMENTS of the respective dtype); io == NULL means float32
 * everywhere.  params_out stays float32. */
int hk_fit_apply_io(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const void* src, int64_t src_stride,
                    const void* ref, int64_t ref_stride, int32_t height, int32_t width, const double* norm_in,
                    float* params_out /* nullable */, int32_t n_param_bands, void* corr_out /* nullable */,
                    double* norm_out, uint64_t* r2_fail_count);

/* Where the outputs of a block go when the caller keeps whole rasters on the host (homonim/fuse.py:310-319 writes the
 * out-block of every block into the corrected / parameter files, raster_array.py:478-491 crops the halo): rows
 * [row0, row0 + rows) x columns [col0, col0 + cols) of the block are copied to corr_out / params_out, whose rows are
 * `stride` elements apart and whose parameter planes `band_stride` elements -- i.e. corr_out points at the pixel of
 * the caller's raster where the window's first pixel belongs. */
typedef struct hk_out_window {
    int64_t stride;       /* elements between rows of corr_out (and of params_out unless param_stride is set); >= cols */
    int64_t band_stride;  /* elements between the planes of params_out */
    int32_t row0, col0;   /* first row / column of the block that is written */
    int32_t rows, cols;   /* size of the written window */
    int64_t param_stride; /* elements between rows of params_out when it differs from corr_out's; 0: `stride` serves both */
} hk_out_window;

/* hk_fit_apply_io with an output window: the block loop of RasterFuse.process (homonim/fuse.py:295-319) per call --
 * read-block in, out-block of the corrected raster (and of the parameters) out, straight into the caller's arrays.
 * When src / ref / corr_out / params_out are page-locked (hk_host_alloc / hk_host_register) the copies are asynchronous
 * and the call synchronises its stream once; calls from several threads overlap their transfers and kernels. */
int hk_fit_apply_block(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const void* src, int64_t src_stride,
                       const void* ref, int64_t ref_stride, int32_t height, int32_t width, const double* norm_in,
                       float* params_out, int32_t n_param_bands, void* corr_out, const hk_out_window* window,
                       double* norm_out, uint64_t* r2_fail_count);

/* hk_fit_apply_block that also returns the validity of the corrected window.  valid_out (nullable: then this IS
 * hk_fit_apply_block, launch for launch): one byte per pixel of the window, 255 where the float32 corrected value is not NaN and
 * 0 where it is -- the mask of the reference's corrected RasterArray (what RasterArray.to_rio_dataset hands to write_mask when the
 * output has no nodata value, homonim/raster_array.py:493-500), taken BEFORE the conversion to the output dtype, so it carries the
 * source mask, the r2 in-painting and (the two-grid forms) mask_partial as the corrected block has them.  Its rows lie
 * window->stride BYTES apart (the validity raster has the corrected raster's width), packed without a window; it needs corr_out.
 * The typed window is bit for bit hk_fit_apply_block's; a float32 output without nodata keeps its NaNs.  One kernel
 * (cast_out_valid_kernel, every output dtype, float32 included) reads the float32 plane once and writes both. */
int hk_fit_apply_block_valid(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const void* src, int64_t src_stride,
                             const void* ref, int64_t ref_stride, int32_t height, int32_t width, const double* norm_in,
                             float* params_out, int32_t n_param_bands, void* corr_out, uint8_t* valid_out,
                             const hk_out_window* window, double* norm_out, uint64_t* r2_fail_count);


/* RefSpaceModel.fit + RefSpaceModel.apply (homonim/kernel_model.py:476-503) of one block pair on DIFFERENT grids of one
 * CRS, entirely on the device -- source and reference blocks in, corrected block (source grid) out:
 *   source --down_resampling--> reference grid; KernelModel.fit there (incl. block statistics / in-painting);
 *   gain, offset --up_resampling--> source grid; re-masked with the source mask, or (mask_partial) with the full-coverage
 *   mask of kernel_model.py:375-409 brought back with `nearest`; KernelModel.apply.
 * down = mapping source <- reference grid (src_col = down[0] * ref_col + down[1], src_row = down[2] * ref_row + down[3]),
 * up = mapping reference <- source grid; both as hk_reproject defines them.  params_out (nullable): n_param_bands planes on
 * the REFERENCE grid.  io (nullable) types src / ref / corr_out as in hk_fit_apply_io. */
typedef struct {
    double down[4];
    double up[4];
    int32_t down_resampling;  /* rasterio.enums.Resampling value, KernelModel._get_resampling(src.res, ref.res) */
    int32_t up_resampling;    /* KernelModel._get_resampling(param.res, src.res) */
    int32_t mask_partial;
} hk_space_desc;
int hk_refspace_fit_apply(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_space_desc* space,
                          const void* src, int64_t src_stride, int32_t src_height, int32_t src_width, const void* ref,
                          int64_t ref_stride, int32_t ref_height, int32_t ref_width, float* params_out,
                          int32_t n_param_bands, void* corr_out, uint64_t* r2_fail_count);
/* ... and the validity of the corrected block, src_height x src_width bytes, packed (valid_out nullable; see
 * hk_fit_apply_block_valid) */
int hk_refspace_fit_apply_valid(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_space_desc* space,
                                const void* src, int64_t src_stride, int32_t src_height, int32_t src_width, const void* ref,
                                int64_t ref_stride, int32_t ref_height, int32_t ref_width, float* params_out,
                                int32_t n_param_bands, void* corr_out, uint8_t* valid_out, uint64_t* r2_fail_count);

/* SrcSpaceModel.fit + KernelModel.apply (homonim/kernel_model.py:506-535, :442-463) of one block pair on DIFFERENT grids of one
 * CRS, entirely on the device -- source and reference blocks in, corrected block (source grid) out:
 *   reference --resampling--> source grid (destination nodata NaN); KernelModel.fit there (incl. block statistics / in-painting);
 *   all parameter bands masked with the source mask, or (mask_partial) with the full-coverage mask of kernel_model.py:375-409:
 *   the reference's valid mask averaged onto the source grid (>= 1) & "has gain or offset", eroded by (kh+2) x (kw+2) (:526-531);
 *   KernelModel.apply; conversion to the output dtype.
 * map = mapping reference <- source grid (ref_col = map[0] * src_col + map[1], ref_row = map[2] * src_row + map[3]) as hk_reproject
 * defines it.  With `average` the typed reference pixels are read once, by a kernel that forms the averaged value and the
 * coverage fraction together; every other method goes through a float32 copy of the block and hk_reproject's kernels.  The results
 * are bit for bit those of hk_reproject, hk_fit, hk_partial_mask and hk_apply called one after the other.  params_out (nullable):
 * n_param_bands planes on the SOURCE grid.  io (nullable) types src / ref / corr_out as in hk_fit_apply_io. */
typedef struct {
    double map[4];
    int32_t resampling;    /* rasterio.enums.Resampling value, KernelModel._get_resampling(ref.res, src.res) */
    int32_t mask_partial;
} hk_srcspace_desc;
int hk_srcspace_fit_apply(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_srcspace_desc* space,
                          const void* src, int64_t src_stride, int32_t src_height, int32_t src_width, const void* ref,
                          int64_t ref_stride, int32_t ref_height, int32_t ref_width, float* params_out,
                          int32_t n_param_bands, void* corr_out, uint64_t* r2_fail_count);
/* ... and the validity of the corrected block, src_height x src_width bytes, packed (valid_out nullable; see
 * hk_fit_apply_block_valid) */
int hk_srcspace_fit_apply_valid(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_srcspace_desc* space,
                                const void* src, int64_t src_stride, int32_t src_height, int32_t src_width, const void* ref,
                                int64_t ref_stride, int32_t ref_height, int32_t ref_width, float* params_out,
                                int32_t n_param_bands, void* corr_out, uint8_t* valid_out, uint64_t* r2_fail_count);

/* Page-lock caller memory so the host-pointer entry points above become truly asynchronous: with pinned src/ref/output
 * arrays the H2D copy, the kernel and the D2H copy of different calls (different host threads, different pooled streams)
 * overlap; with pageable memory HIP stages every copy synchronously.  The reference has no counterpart (its blocks are
 * numpy arrays read by rasterio, homonim/raster_pair.py:331-340). */
int hk_host_alloc(hk_ctx* ctx, size_t bytes, void** hptr);   /* pinned allocation */
int hk_host_free(hk_ctx* ctx, void* hptr);                   /* ctx may be NULL (the memory belongs to no device) */
int hk_host_register(hk_ctx* ctx, void* hptr, size_t bytes); /* pin existing memory in place (usable from every device) */
int hk_host_unregister(hk_ctx* ctx, void* hptr);             /* ctx may be NULL */

/* ------------------------------------------------------------------------------------------------------------------
 * device-resident entry points (inputs already in HBM): what bench.py times and what the streaming tile pipeline
 * is built from.  Buffers come from hk_dev_alloc; planes are height x stride float32 with stride % 4 == 0.
 * A job names its stream by index: jobs on one stream must be issued by one host thread at a time (stream order is the
 * only ordering).  Host-pointer calls (hk_fit, ...) lease the same pooled streams and their scratch buffers; the library
 * keeps the two apart at run time: a lease prefers a stream no device job has used, drains one that was used before taking
 * it, and a device-job call waits while its stream is leased.  Mixing both on one context is therefore safe call by call but
 * serialises them on that stream -- use a second context where they should overlap, and always when a gain-offset job with
 * an r2 threshold runs WITHOUT hk_dev_job.scratch: between its hk_fit_apply_dev and its hk_inpaint_dev* the in-painting's
 * inputs live in the stream's own scratch, which a host-pointer call leasing that stream would overwrite.
 */
int hk_dev_alloc(hk_ctx* ctx, size_t bytes, void** dptr);
int hk_dev_free(hk_ctx* ctx, void* dptr);
int hk_memcpy_h2d(hk_ctx* ctx, void* dst, const void* src, size_t bytes);
int hk_memcpy_d2h(hk_ctx* ctx, void* dst, const void* src, size_t bytes);
int hk_memset(hk_ctx* ctx, void* dst, int value, size_t bytes);

typedef struct {
    const float* src;      /* device, n_bands planes */
    const float* ref;      /* device, n_bands planes */
    float* gain;           /* device, nullable */
    float* offset;         /* device, nullable */
    float* r2;             /* device, nullable (written only when the R2 variant runs) */
    float* corr;           /* device, nullable */
    const double* norm;    /* device, n_bands x 2 float64 (gain-blk-offset), else NULL */
    uint64_t* fail_count;  /* device, n_bands counters (must be zeroed by the caller), nullable */
    int32_t n_bands;
    int32_t height, width;
    int64_t stride;        /* elements between rows, all planes */
    int64_t band_stride;   /* elements between band planes, all arrays */
    int32_t seg_rows;      /* rows per wave segment; 0 = library default */
    int32_t stream;        /* index into the context's stream pool */
    /* Store window of hk_fit_apply_dev, in job coordinates: only these rows / columns of the job are written (and counted).
     * A block of a larger device-resident raster is processed in place -- src / ref / corr point at the block's first
     * pixel INCLUDING its halo, height / width are the in-block's -- and only its out-block is stored: the halo crop of
     * homonim/raster_array.py:478-491 as homonim/fuse.py:310-312 applies it.  All zero = the whole job.  out_col0 and
     * out_col0 + out_cols must be multiples of 4 (or end at the job's last column).  Not with r2_inpaint_thresh. */
    int32_t out_row0, out_col0, out_rows, out_cols;
    /* Optional device scratch for gain-offset with an r2 threshold (else NULL / 0): hk_dev_job_scratch_bytes() bytes,
     * 16-byte aligned, owned by the caller and tied to this job until its hk_inpaint_dev / hk_inpaint_dev_counts.  A job that
     * carries it gets the in-painting's inputs left there by hk_fit_apply_dev -- offsets and the one-byte source flags
     * (r2 > thresh) & (gain > 0) & valid (kernel_model.py:363), 5 bytes per pixel of stores -- and the in-painting starts from
     * them instead of running the fit once more: provide it where pixels are expected to fail the r2 mask (real imagery:
     * block after block), leave it NULL where they are not (the fit then runs its lighter build and moves 12 bytes per pixel). */
    void* scratch;
    uint64_t scratch_bytes;
} hk_dev_job;
/* Size of hk_dev_job.scratch for a job of this shape (5 bytes per pixel of the job's planes incl. row / band padding). */
uint64_t hk_dev_job_scratch_bytes(int32_t n_bands, int32_t height, int64_t stride, int64_t band_stride);

/* Launch the fused kernel over all bands of a device-resident job (asynchronous on stream `job->stream`).  With an r2
 * threshold the pixels failing the mask are only COUNTED (job->fail_count); follow with hk_inpaint_dev. */
int hk_fit_apply_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job);
/* Second half of gain-offset with an r2 threshold on a device-resident job (kernel_model.py:361-371): waits for the
 * stream, reads job->fail_count and, for every band with failing pixels, in-paints their offsets and re-runs the fit
 * with them (recomputed gains, re-applied correction; parameter planes of the job are updated when present).  A no-op
 * for the other models.  *n_fail_out (nullable) receives the number of failing pixels over all bands; the counters
 * are then cleared (asynchronously), ready for the job's next hk_fit_apply_dev.  Returns after queueing the passes on
 * `job->stream`. */
int hk_inpaint_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, uint64_t* n_fail_out);
/* The same in two halves, for pipelines that must not drain the stream after every launch: hk_fail_counts_async queues the
 * copy of the job's counters into `host_counts` (n_bands values, pinned host memory: hk_host_alloc), their clearing and
 * the recording of `ready`; after hk_event_sync(ready) the caller passes the counts to hk_inpaint_dev_counts, which only
 * queues work.  Launch N + 1 (into a second counter buffer) may be queued before the counts of launch N are looked at.
 * Pass the counts on unchanged.  (Up to ABI version 5 a raw counter could carry HK_COUNT_RETRY instead of a count: the lighter
 * kernel build such jobs start with voided the whole band when it could not settle a wave-row.  Since version 6 that build marks
 * the wave-rows it leaves open and a second launch of the complete build does exactly those: every counter is a count.  The
 * constant stays defined for consumers written against the older header; the library never sets it.) */
#define HK_COUNT_RETRY (1ull << 63)
int hk_fail_counts_async(hk_ctx* ctx, const hk_dev_job* job, uint64_t* host_counts, hk_event* ready);
/* 1 when the counts of a launch call for its second half (hk_inpaint_dev_counts): some band has failing pixels; 0 when the
 * launch's outputs are final.  Callers need not interpret the raw counters (host-only, no device call). */
int hk_counts_pending(const uint64_t* counts, int32_t n_bands);
int hk_inpaint_dev_counts(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, const uint64_t* counts,
                          uint64_t* n_fail_out);
/* Per-band block normalisation on device planes -> norm (device, n_bands x 2 float64); asynchronous. */
int hk_block_norm_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, double* norm_dev);
/* BATCHED launches: `n_jobs` device-resident jobs -- the block positions of a resident mosaic (homonim/raster_pair.py:342-428
 * yields them one by one and homonim/fuse.py:395-404 hands each to a thread), the tiles of a tile list -- as ONE launch per
 * kernel stage on jobs[0].stream (all jobs name that stream) instead of one launch, and one launch tail, per job.  Jobs may
 * differ in shape, planes and store window; they share `desc` and ask for the same set of outputs (the same pointers are NULL in
 * every job).  Results are bit-identical to the per-job calls: a job's statistics and wave units do not depend on the launch it
 * travels in.  hk_block_norm_batch_dev writes the jobs' statistics one after the other (job 0's n_bands x 2 float64, then job
 * 1's, ...) into norm_dev; hk_fit_apply_batch_dev reads each job's own `norm` pointer (point it into that buffer).  With an r2
 * threshold every job keeps its own fail_count / scratch and is finished by its own hk_inpaint_dev* call, as after
 * hk_fit_apply_dev.  The job tables travel through a small ring of pinned staging buffers of the stream: the calls only queue
 * work.  One fused launch exists for gain-blk-offset without R2 (the block-partitioned mosaic, where it pays); for the other
 * models hk_fit_apply_batch_dev queues the jobs' launches one after the other -- the job-table look-up at the start of every
 * wave costs their short waves more than the launches it saves.  Limits: 65536 jobs, 32767 planes (jobs x bands) per statistics
 * batch; the statistics workspace of the stream grows to planes x (190 KB + 8 % of the largest plane). */
int hk_block_norm_batch_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* jobs, int32_t n_jobs, double* norm_dev);
int hk_fit_apply_batch_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* jobs, int32_t n_jobs);
/* hk_fail_counts_async for the jobs of a batch: their counters, job after job (sum of n_bands values), into the pinned
 * `host_counts`, cleared on the device, ONE event.  Pass each job its own slice to hk_inpaint_dev_counts afterwards. */
int hk_fail_counts_batch_async(hk_ctx* ctx, const hk_dev_job* jobs, int32_t n_jobs, uint64_t* host_counts, hk_event* ready);
/* The same statistics (KernelModel._fit_block_norm, homonim/kernel_model.py:216-229) for a block whose ROWS are spread over
 * `world_size` ranks / devices -- the optional collective of a gain-blk-offset block too large for one GPU.  `job` is this
 * rank's slab of the block (any number of rows, the block's width).  Phases 0..5 are queued one at a time on job->stream;
 * between two phases the caller waits for the stream and all-reduces (SUM, float64) the exchange buffer `xchg_dev` over the
 * ranks (RCCL: torch.distributed.all_reduce on a tensor that owns the buffer; homonim_amd/split_norm.py), all ranks in step.
 * The buffer holds hk_block_norm_split_exchange_doubles(n_bands) values: the slabs' shifts, then their moments, then the
 * three histogram levels of the exact radix select (integer counts, exact in float64).  After phase 5 `norm_dev`
 * (n_bands x 2 float64, device) holds the block's norm, identical on every rank: order statistics exactly those of the whole
 * block, std ratio equal to the single-device value up to the order of the float64 sums. */
uint64_t hk_block_norm_split_exchange_doubles(int32_t n_bands);
int hk_block_norm_split_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, int32_t phase, int32_t world_size,
                            double* xchg_dev, double* norm_dev);
/* The same with the all-reduces done by the library: RCCL over xGMI, queued on job->stream between the phases -- no host
 * synchronisation, no tensor library in the data path (BASELINE.json north_star: "RCCL over xGMI only for the optional
 * block-mean offset reduction").  One process per GPU; every rank creates its context, joins the communicator once
 * (hk_comm_init) and then calls hk_block_norm_split_comm_dev with its slab of each block, all ranks in the same order.
 *   hk_comm_unique_id : rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other ranks through whatever
 *                       launched them (a file, the torch.distributed store, MPI ...: homonim_amd/dist.py init_comm).
 *   hk_comm_init      : collective over the ranks (ncclCommInitRank); one communicator per context.
 *   hk_block_norm_split_comm_dev : asynchronous; norm_dev (n_bands x 2 float64, device) is valid in stream order and
 *                       identical on every rank.  A slab may have no rows (height 0): the rank contributes zeros.
 *                       A block of 2^32 or more valid pixels gets NaN statistics on every rank (32-bit histogram bins).
 *   hk_comm_allreduce_f64_dev : in-place SUM of a device buffer over the communicator on a pooled stream (the primitive
 *                       above; exported for callers with their own phase loop).
 * librccl is opened at run time on first use (HK_ERR_UNSUPPORTED if it is absent). */
#define HK_COMM_ID_BYTES 128
int hk_comm_unique_id(uint8_t id[HK_COMM_ID_BYTES]);
int hk_comm_init(hk_ctx* ctx, const uint8_t id[HK_COMM_ID_BYTES], int32_t rank, int32_t world_size);
int hk_comm_destroy(hk_ctx* ctx);
int hk_comm_info(hk_ctx* ctx, int32_t* rank, int32_t* world_size);   /* rank -1 / world 0: no communicator */
int hk_comm_allreduce_f64_dev(hk_ctx* ctx, double* buf_dev, uint64_t count, int32_t stream);
int hk_block_norm_split_comm_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, double* norm_dev);
/* The masked sums of RasterCompare.process / get_block_sums (homonim/compare.py:243-255) on the job's src and ref planes
 * (job->corr etc. are not used), per band into sums_dev (device, n_bands x 7 float64; asynchronous):
 *   [ sum src, sum ref, sum src^2, sum ref^2, sum src*ref, sum (ref - src)^2, number of pixels ]
 * over the pixels valid in both rasters.  Per-pixel terms are formed in float32 as numpy does on float32 arrays; they are
 * accumulated in float64 in a fixed order (the reference's float32 pairwise sums differ from these by ~1e-7 relative).
 * r2 / RMSE / rRMSE follow from them as in compare.py:142-160. */
int hk_compare_sums_dev(hk_ctx* ctx, const hk_dev_job* job, int32_t src_nodata_mode, float src_nodata,
                        int32_t ref_nodata_mode, float ref_nodata, double* sums_dev);
/* The masked statistics of ParamStats.stats / get_block_sums (homonim/stats.py:217-229) of `n_bands` device-resident float32
 * planes (plane b at planes_dev + b * band_stride, `stride` elements between rows; any parameter raster will do, not only a
 * job's) in ONE launch on pooled stream `stream`, per band into stats_dev (device, n_bands x 10 float64; asynchronous, no host
 * synchronisation):
 *   [ min, max, sum x, sum x^2, N, N(x < thresh), col_min, row_min, col_max, row_max ]
 * over the pixels valid under (nodata_mode, nodata) with utils.nan_equals semantics; the last four are the bounding box of the
 * valid pixels (stats.py:135-173).  Every pixel term is (double)x resp. (double)x * (double)x (exact), accumulated in float64
 * in a fixed order: bit-identical run to run and to hk_param_stats on the same plane.  min / max are the float32 values, the
 * counts are exact (64-bit, returned as doubles), x < thresh is decided in float64 (a NaN thresh counts nothing); +-inf
 * pixels are data.  Under HK_NODATA_NONE / HK_NODATA_VALUE a NaN pixel is valid and makes min, max and both sums NaN, as in
 * numpy.  A band without a valid pixel gives [ +inf, -inf, 0, 0, 0, 0, width, height, -1, -1 ].  16-byte loads are used when
 * planes_dev is 16-byte aligned and stride and band_stride are multiples of 4; any other layout is accepted and gives the same
 * bits.  mean / std / Inpaint (%) follow as in stats.py:175-192. */
int hk_param_stats_dev(hk_ctx* ctx, const float* planes_dev, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                       int64_t band_stride, int32_t stream, int32_t nodata_mode, float nodata, double thresh, double* stats_dev);

/* Average overviews (the internal overviews of homonim/fuse.py:152-165: factors 2, 4, ... with Resampling.average) of `n_bands`
 * device-resident planes of sample type `dtype` (hk_dtype), all levels from one pass over the source, on pooled stream `stream`
 * (asynchronous).  Level m = 1..n_levels has shape (ceil(height / 2^m), ceil(width / 2^m)) and is written to out_dev[m - 1]
 * (device; strides in elements).  It is computed from level m - 1 as stored (level 0 = the raster), as GDAL cascades `average`:
 * pixel (i, j) takes the pixels (2i..2i+1, 2j..2j+1) of level m - 1 that lie inside it and are valid under (nodata_mode, nodata)
 * -- HK_NODATA_NONE: all, a NaN is data and propagates; HK_NODATA_NAN: not NaN (every pixel of an integer type); HK_NODATA_VALUE:
 * not equal to `nodata` (an integer type: a value of the type; float32: compared after rounding it to float32).  A cell without
 * a valid pixel gives nodata.  float32: the valid values are summed as float64 in row-major order, divided by their count in
 * float64 and rounded once to float32 -- bit-identical to hk_reproject with Resampling.average on the mapping (2, 0, 2, 0);
 * float64: the same without the rounding; integer types: floor((2 S + n) / (2 n)) of the exact sum S of the n valid values
 * (round half up, GDAL's + 0.5).  GDAL >= 3.3 weights fractional source pixels where a dimension is odd; whole cells clipped at
 * the edge are used here (the two agree for even sizes).  16-byte loads are used where the planes allow it; any other layout
 * gives the same bits.  n_levels <= 31; a level past 1 x 1 repeats it. */
int hk_overviews_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                     int64_t stride, int64_t band_stride, int32_t nodata_mode, double nodata, int32_t n_levels,
                     void* const out_dev[], const int64_t out_stride[], const int64_t out_band_stride[], int32_t stream);

/* hk_overviews_dev under a validity plane: valid_dev holds one byte per pixel of the raster (valid where not 0; valid_stride bytes
 * between rows; one plane for all bands).  Level m's pixel (i, j) takes the pixels of level m - 1 that lie inside its 2 x 2 cell AND
 * are valid, with the arithmetic above: float types the float64 sum in row-major order divided by the count and rounded once,
 * integer types floor((2 S + n) / (2 n)).  A NaN under a valid byte is data and propagates, as under HK_NODATA_NONE.  A cell
 * without a valid pixel gives 0 (integer types) or NaN (float types).  The same pass writes level m's own validity to
 * out_valid_dev[m - 1] (out_valid_stride[m - 1] bytes between rows): 255 where the cell had a valid pixel, else 0; level m + 1
 * cascades from level m's values and validity as stored.  16-byte loads of the samples and whole-word loads of the validity are
 * used where the planes allow it (valid_dev and its stride multiples of 16); any other layout gives the same bits. */
int hk_overviews_valid_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                           int64_t stride, int64_t band_stride, const uint8_t* valid_dev, int64_t valid_stride, int32_t n_levels,
                           void* const out_dev[], const int64_t out_stride[], const int64_t out_band_stride[],
                           uint8_t* const out_valid_dev[], const int64_t out_valid_stride[], int32_t stream);

/* hk_dataset_mask for device-resident planes (band b at planes_dev + b * band_stride elements, out_dev + b * out_band_stride),
 * mask and output: one launch for all bands -- a lane reads the validity of 8 consecutive pixels once and loops the bands inside.
 * Whole groups of 8 pixels move as 8- / 16-byte loads and 16-byte stores where a plane row starts at a multiple of min(16, 8 x
 * sample size) bytes and the output row at a multiple of 16; any other layout gives the same bits pixel by pixel.  planes_dev and
 * an alpha plane are aligned to their sample size, out_dev to 4.  Queued on pooled stream `stream`; asynchronous. */
int hk_dataset_mask_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                        int64_t stride, int64_t band_stride, const void* mask_dev, int32_t mask_kind, int64_t mask_stride,
                        float* out_dev, int64_t out_stride, int64_t out_band_stride, int32_t stream);

/* The typed prefill of a device-resident raster, as RasterFuse._allocate fills the host raster (numpy.full): `value` -- NaN allowed
 * for HK_DTYPE_F32 / HK_DTYPE_F64, otherwise a value the sample type holds -- into `width` samples of each of `height` rows of
 * `n_bands` planes of `dtype` (band b at planes_dev + b * band_stride elements, rows `stride` elements apart).  Nothing of the row
 * padding (stride - width samples) and nothing between planes is written.  planes_dev is aligned to the sample size; all index
 * arithmetic is 64-bit.  Whole 16-byte units of a row are one store, wherever the row starts.  Queued on pooled stream `stream`;
 * asynchronous.  HK_ERR_ARG: a NULL pointer, an unknown dtype, a size below 1, stride < width, a negative band_stride, a plane
 * that overlaps the next, a value the type does not hold. */
int hk_fill_planes_dev(hk_ctx* ctx, void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                       int64_t band_stride, double value, int32_t stream);

/* A window of a device-resident raster that may reach beyond it, all bands in one launch: what the reference's boundless read
 * gives (RasterArray.from_rio_dataset, homonim/raster_array.py:172-188).  `planes_dev`: n_bands x height x width samples of `dtype`
 * on `stride` / `band_stride` (elements); the window is (row_off, col_off, out_height, out_width) in raster coordinates, offsets
 * may be negative and the window may miss the raster altogether.  nodata_mode HK_NODATA_VALUE: out_dev holds samples of `dtype`,
 * the raster's inside it and `nodata` (a value the type holds) outside; HK_NODATA_NONE / HK_NODATA_NAN: out_dev holds float32, the
 * plain value conversion of the raster's samples inside (exact for 8/16-bit integers, round to nearest for 32-bit integers and
 * float64; a float32 keeps its bits) and NaN (0x7FC00000) outside, `nodata` is not read.  Band b of the window goes to out_dev +
 * b * out_band_stride, rows out_stride apart (elements of the output's type); nothing outside [row, row + out_width) of it is
 * written and nothing outside the raster is read.  16-byte loads where a unit of a raster row lies inside the raster, sample by
 * sample at the ragged ends; all index arithmetic is 64-bit.  Queued on pooled stream `stream`; asynchronous.  HK_ERR_ARG: a NULL
 * pointer, an unknown dtype or nodata mode, a size below 1, a stride smaller than its width, a negative band stride, planes that
 * overlap, a nodata the type does not hold, a pointer not aligned to its sample size. */
int hk_boundless_window_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                            int64_t stride, int64_t band_stride, int32_t row_off, int32_t col_off, int32_t out_height,
                            int32_t out_width, int32_t nodata_mode, double nodata, void* out_dev, int64_t out_stride,
                            int64_t out_band_stride, int32_t stream);

/* Free and total bytes of the context's device as the runtime reports them (hipMemGetInfo): what a caller that is about to make
 * whole rasters resident compares its needs with.  Either pointer may be NULL. */
int hk_dev_mem_info(hk_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);

/* hk_deflate_tiles for device-resident planes: streams, offsets and sizes stay on the device (out_dev of out_capacity >=
 * hk_deflate_bound's bytes; tile_offsets_dev: n_tiles + 1, tile_sizes_dev: n_tiles int64).  Queued on pooled stream `stream`;
 * asynchronous.  The whole raster is one launch: at most 2^31 - 1 chunks. */
int hk_deflate_tiles_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                         int64_t stride, int64_t band_stride, int32_t tile, void* out_dev, int64_t out_capacity,
                         int64_t* tile_offsets_dev, int64_t* tile_sizes_dev, int32_t stream);
/* hk_deflate_tiles_dev with a predictor, as hk_deflate_tiles_pred states it; predictor 1 gives the bytes of hk_deflate_tiles_dev. */
int hk_deflate_tiles_pred_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                              int64_t stride, int64_t band_stride, int32_t tile, void* out_dev, int64_t out_capacity,
                              int64_t* tile_offsets_dev, int64_t* tile_sizes_dev, int32_t stream, int32_t predictor);

/* hk_inflate_image for device-resident streams, offsets and sizes: the raster into out_dev, the statuses into status_dev (n_blocks
 * int32, required: nothing comes back to the host, so the call cannot report a refused block itself); work_dev: hk_inflate_bound's
 * work_bytes, 16-byte aligned.  A negative offset or a size below 1 gives the block HK_INFLATE_TRUNCATED; at most 256 MiB of a stream
 * are looked at.  Queued on pooled stream `stream`; asynchronous.  One launch: at most 2^31 - 1 blocks. */
int hk_inflate_image_dev(hk_ctx* ctx, const hk_inflate_layout* layout, const void* streams_dev, const int64_t* offsets_dev,
                         const int64_t* sizes_dev, void* work_dev, void* out_dev, int64_t stride, int64_t band_stride,
                         int32_t* status_dev, int32_t stream);
/* hk_inflate_image_dev for LZW streams (hk_lzw_image): the statuses are HK_LZW_*, a stream that is not there HK_LZW_TRUNCATED. */
int hk_lzw_image_dev(hk_ctx* ctx, const hk_inflate_layout* layout, const void* streams_dev, const int64_t* offsets_dev,
                     const int64_t* sizes_dev, void* work_dev, void* out_dev, int64_t stride, int64_t band_stride,
                     int32_t* status_dev, int32_t stream);

/* hk_refspace_fit_apply_valid / hk_srcspace_fit_apply_valid on device-resident rasters: source and reference blocks on DIFFERENT
 * grids of one CRS, many bands per call, typed planes on the caller's strides, store windows, a named stream, caller-owned scratch.
 * The result is the host form's, byte for byte: for every band b, the planes the host entry returns for that band's blocks under
 * the same desc, io and space, cut to the windows, lie in corr, valid and params afterwards; nothing outside the windows, between
 * rows or between planes is written.  Both forms run one chain of launches (the host form is staging in, that chain, staging out),
 * so no allowance is involved.
 *   Strides  : any value >= the width; planes are aligned to their element only, and of a plane's last row only `width` elements
 *              need to exist: nothing past a row's last pixel is read.  Every input plane is brought into scratch laid out as the
 *              host form lays out its slab: float32 by a strided device copy, another dtype by the conversion kernel -- which
 *              reads whole quads of a row, so it reads the caller's plane only where the width is a multiple of 4 and a strided
 *              device copy of the plane (in scratch) otherwise.  The SrcSpace chain's reference under `average` is read where it
 *              lies, pixel by pixel, whatever its dtype and stride.  All address arithmetic is 64-bit: planes may lie 2^32
 *              elements and more apart.
 *   Windows  : act at the last stage only -- the whole block is computed (in-painting and mask_partial need it), converted to the
 *              output dtype in scratch (the conversion kernels store whole quads of a row, so they do not write into the caller's
 *              raster), and the windows of the corrected, validity and parameter planes are put in place by strided device copies.
 *   Bands    : run one after the other in stream order on job->stream and share one band's worth of scratch.
 *   Waiting  : the call only queues work and returns, except for gain-offset with an r2 threshold, where it waits for the stream once
 *              per band to read that band's failure count (and in-paints where it is not 0, as hk_fit does).  n_fail_out[b] is that
 *              count, and 0 for every other configuration.  The in-painting's own workspace is the stream's, never `scratch`.
 *   Streams  : hk_dev_job's rules apply unchanged -- jobs on one stream are issued by one host thread at a time, host-pointer calls
 *              lease the same pooled streams, and a call waits while its stream is leased.  With scratch == NULL the slab is the
 *              stream's own staging slab, grown as needed (growing it waits for the stream).
 *   Refusals : before anything is launched; the host form's status and text wherever the check is shared.  Also HK_ERR_ARG:
 *              n_bands < 1; reserved not 0; n_param_bands not what the model configuration gives (with params); a stride below its width (or its
 *              window's); band strides that make planes overlap; a window outside its grid; valid without corr; a stream index
 *              outside the pool; scratch not 256-byte aligned or smaller than hk_*_dev_scratch_bytes() (the text names the size).
 * hk_*_dev_scratch_bytes: the size of `scratch` for this call (a multiple of 256), 0 for arguments the entry would refuse; the
 * job's own scratch fields are not looked at.  Plain host arithmetic (no device needed). */
typedef struct {
    const void* src;      /* device: n_bands planes of io->src_dtype (float32 when io is NULL), first pixel of the source block */
    const void* ref;      /* device: n_bands planes of io->ref_dtype, first pixel of the reference block */
    void* corr;           /* device: io->out_dtype; the place of the corrected WINDOW's first pixel in the caller's raster */
    uint8_t* valid;       /* device, nullable: n_bands planes, 255 / 0 as hk_fit_apply_block_valid defines; the same window */
    float* params;        /* device, nullable: parameter p of band b is the plane params + (p * n_bands + b) * param_band_stride
                             (the band order of the reference's parameter file); the place of the PARAMETER window's first pixel */
    int64_t src_stride, src_band_stride, ref_stride, ref_band_stride;        /* elements of the respective dtype */
    int64_t corr_stride, corr_band_stride, valid_stride, valid_band_stride;  /* valid_*: bytes */
    int64_t param_stride, param_band_stride;
    int32_t n_bands, n_param_bands;
    int32_t src_height, src_width, ref_height, ref_width;
    int32_t out_row0, out_col0, out_rows, out_cols;  /* window of the source-grid block stored to corr / valid; all 0: the whole block */
    int32_t par_row0, par_col0, par_rows, par_cols;  /* window of the parameter grid (refspace: the reference block's; srcspace: the
                                                        source block's) stored to params; all 0: the whole grid */
    int32_t stream;       /* index into the context's stream pool, as in hk_dev_job */
    int32_t reserved;     /* 0 */
    void* scratch;        /* device, nullable: hk_*_dev_scratch_bytes() bytes, 256-byte aligned, the caller's until the stream has
                             passed this call; NULL: the stream's own scratch, grown as needed */
    uint64_t scratch_bytes;
} hk_two_grid_job;
uint64_t hk_refspace_dev_scratch_bytes(const hk_fit_desc* desc, const hk_io_desc* io, const hk_space_desc* space,
                                       const hk_two_grid_job* job);
uint64_t hk_srcspace_dev_scratch_bytes(const hk_fit_desc* desc, const hk_io_desc* io, const hk_srcspace_desc* space,
                                       const hk_two_grid_job* job);
int hk_refspace_fit_apply_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io /* nullable */, const hk_space_desc* space,
                              const hk_two_grid_job* job, uint64_t* n_fail_out /* host, nullable: n_bands counts */);
int hk_srcspace_fit_apply_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io /* nullable */,
                              const hk_srcspace_desc* space, const hk_two_grid_job* job, uint64_t* n_fail_out);

/* HIP events on the pooled streams, so callers time exactly the stream the kernels run on. */
int hk_event_create(hk_ctx* ctx, hk_event** ev);
int hk_event_destroy(hk_ctx* ctx, hk_event* ev);
int hk_event_record(hk_ctx* ctx, hk_event* ev, int32_t stream);
int hk_stream_wait_event(hk_ctx* ctx, int32_t stream, hk_event* ev); /* work queued on `stream` after this call waits for the event (device side) */
int hk_event_sync(hk_ctx* ctx, hk_event* ev);  /* blocks the calling thread until the event has happened */
int hk_event_elapsed_ms(hk_ctx* ctx, hk_event* start, hk_event* stop, float* ms); /* syncs on `stop` */
int hk_stream_sync(hk_ctx* ctx, int32_t stream);

/* Self-test of the cross-lane primitives the kernels rely on (DPP wave shifts); 0 = pass. */
int hk_selftest(hk_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* HOMONIM_HK_H */
