"""
Block scheduler + ``RasterFuse`` surface for the MI355X hot path.

The reference's ``RasterFuse.process`` (homonim/fuse.py:321-408) walks (band x spatial block) work items produced by
``RasterPairReader.block_pairs`` (homonim/raster_pair.py:342-428) and, per item, runs ``read -> model.fit ->
model.apply -> write`` on a thread pool (fuse.py:295-319,396-408).  This module keeps that call surface -- the
``process()`` signature and the three configuration dict factories -- on in-memory same-grid rasters:

* ``auto_block_shape`` / ``block_pairs`` reproduce the reference partition exactly (halve the longer side until a
  block fits ``max_block_mem``, overlap = ceil(kernel/2)), because ``gain-blk-offset`` results depend on it
  (its normalisation statistics are taken over each in-block, kernel_model.py:216-229);
* every block is one fused fit+apply kernel launch through the C ABI; worker threads check streams out of the
  context pool so H2D / kernel / D2H of different blocks overlap (ctypes releases the GIL);
* blocks are independent: they shard round-robin over the GPUs of a node (one context per device inside one process)
  and/or over ranks (one process per GPU), with no data-path collective.

Rasters may also be given / written as GeoTIFF paths (homonim_amd/tiff.py: the classic-TIFF subset the reference's
rasters use).  A source and a reference in different CRSs are brought together as the reference's
``utils.same_orientation_crs`` does (homonim/utils.py:190-209): the processing-grid image is warped, bilinear, into the other's
CRS on the device (hk_warp.hip; the CRSs homonim_amd/crs.py knows), everything after that runs on one CRS.  Band matching by
wavelength stays outside (GDAL).
"""
import math
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from homonim_amd import _hk, utils
from homonim_amd import crs as crs_defs
from homonim_amd.enums import Model, ProcCrs, Resampling
from homonim_amd.errors import BlockSizeError, ConfigWarning, DeviceError, ImageFormatWarning, IoError
from homonim_amd.geo import Affine, CRS, Window, is_rotated, pixel_size, suggested_warp_grid
from homonim_amd.kernel_model import KernelModel, RefSpaceModel, SrcSpaceModel
from homonim_amd.raster_array import RasterArray


class BlockPair(NamedTuple):
    """ Matching block windows of a source / reference pair (homonim/raster_pair.py:45-58). """
    band_i: int
    src_in_block: Window   # overlapping window that is read
    ref_in_block: Window
    src_out_block: Window  # non-overlapping window that is written
    ref_out_block: Window
    outer: bool            # the in-block touches the image boundary


def auto_block_shape(shape: Tuple[int, int], max_block_mem: float = math.inf, dtype_size: int = 4) -> Tuple[int, int]:
    """
    Block (rows, cols) for an image of ``shape``: keep halving the longer side (rows on ties) until a float32 block
    fits ``max_block_mem`` megabytes (2**20 bytes); <= 0 or inf = whole image (homonim/raster_pair.py:227-269 with
    equal source / reference resolutions, i.e. mem_scale 1).
    """
    limit = math.inf if (max_block_mem is None or max_block_mem <= 0) else float(max_block_mem) * 2 ** 20
    rows, cols = float(shape[0]), float(shape[1])
    while rows * cols * dtype_size > limit:
        if rows >= cols:
            rows /= 2
        else:
            cols /= 2
    if rows < 1 or cols < 1:
        raise BlockSizeError("The auto block shape is smaller than a pixel.  Increase 'max_block_mem'.")
    block = (int(math.ceil(rows)), int(math.ceil(cols)))
    if (block[0] < 256 or block[1] < 256) and (block[0] < shape[0] or block[1] < shape[1]):
        import warnings
        warnings.warn(
            f'The auto block shape is small: {block}.  Increase `max_block_mem` to improve processing times.',
            category=ConfigWarning
        )
    return block


def block_pairs(shape: Tuple[int, int], n_bands: int, overlap: Tuple[int, int] = (0, 0),
                max_block_mem: float = math.inf) -> Iterator[BlockPair]:
    """
    (band x block) work items in the reference's order: bands outermost, then blocks row-major
    (homonim/raster_pair.py:379-428).  In-blocks overlap their neighbours by ``overlap`` on every side and are clipped
    to the image; out-blocks tile the image exactly.
    """
    height, width = int(shape[0]), int(shape[1])
    ov_r, ov_c = int(overlap[0]), int(overlap[1])
    blk_r, blk_c = auto_block_shape((height, width), max_block_mem)
    if blk_r <= ov_r or blk_c <= ov_c:
        raise BlockSizeError('The auto block shape is smaller than the overlap.  Increase `max_block_mem`.')
    row_starts = range(-ov_r, height - ov_r, blk_r)
    col_starts = range(-ov_c, width - ov_c, blk_c)
    for band_i in range(n_bands):
        for r0 in row_starts:
            for c0 in col_starts:
                in_r0, in_c0 = max(r0, 0), max(c0, 0)
                in_r1, in_c1 = min(r0 + blk_r + 2 * ov_r, height), min(c0 + blk_c + 2 * ov_c, width)
                out_r0, out_c0 = max(r0 + ov_r, 0), max(c0 + ov_c, 0)
                out_r1, out_c1 = min(r0 + blk_r + ov_r, height), min(c0 + blk_c + ov_c, width)
                outer = in_r0 <= 0 or in_c0 <= 0 or in_r1 >= height or in_c1 >= width
                win_in = Window(in_c0, in_r0, in_c1 - in_c0, in_r1 - in_r0)
                win_out = Window(out_c0, out_r0, out_c1 - out_c0, out_r1 - out_r0)
                yield BlockPair(band_i, win_in, win_in, win_out, win_out, outer)


class Grid(NamedTuple):
    """ A north-up raster grid: geo-transform + size (what the block partition needs of a rasterio dataset). """
    transform: Affine
    height: int
    width: int

    @property
    def res(self) -> Tuple[float, float]:
        return abs(self.transform.a), abs(self.transform.e)

    def window_bounds(self, win: Window) -> Tuple[float, float, float, float]:
        """ (left, bottom, right, top) of a pixel window. """
        t = self.transform
        return (t.c + win.col_off * t.a, t.f + (win.row_off + win.height) * t.e, t.c + (win.col_off + win.width) * t.a,
                t.f + win.row_off * t.e)

    @property
    def bounds(self) -> Tuple[float, float, float, float]:
        return self.window_bounds(Window(0, 0, self.width, self.height))

    def window(self, left: float, bottom: float, right: float, top: float) -> Window:
        """ The (fractional) pixel window of a bounding box. """
        t = self.transform
        return Window((left - t.c) / t.a, (top - t.f) / t.e, (right - left) / t.a, (bottom - top) / t.e)


def expand_window_to_grid(win: Window, expand_pixels: Tuple[int, int] = (0, 0)) -> Window:
    """ The smallest whole-pixel window containing ``win`` grown by ``expand_pixels`` (rows, cols)
    (homonim/utils.py:59-81). """
    col_off = math.floor(win.col_off - expand_pixels[1])
    row_off = math.floor(win.row_off - expand_pixels[0])
    col_frac = (win.col_off - expand_pixels[1]) - col_off
    row_frac = (win.row_off - expand_pixels[0]) - row_off
    width = math.ceil(win.width + 2 * expand_pixels[1] + col_frac)
    height = math.ceil(win.height + 2 * expand_pixels[0] + row_frac)
    return Window(int(col_off), int(row_off), int(width), int(height))


def round_window_to_grid(win: Window) -> Window:
    """ ``win`` with its edges rounded (half to even) to whole pixels (homonim/utils.py:84-101). """
    r0, r1 = round(win.row_off), round(win.row_off + win.height)
    c0, c1 = round(win.col_off), round(win.col_off + win.width)
    return Window(int(c0), int(r0), int(c1 - c0), int(r1 - r0))


def pair_windows(src: Grid, ref: Grid) -> Tuple[Window, Window]:
    """ (src_win, ref_win): the reference window covering the source, and the (possibly boundless) source window covering
    that -- so that blocks re-project between the two grids without losing data (homonim/raster_pair.py:289-291). """
    ref_win = expand_window_to_grid(ref.window(*src.bounds))
    src_win = expand_window_to_grid(src.window(*ref.window_bounds(ref_win)))
    return src_win, ref_win


def resolve_proc_crs(src: Grid, ref: Grid, proc_crs: ProcCrs = ProcCrs.auto) -> ProcCrs:
    """ auto -> the grid with the larger pixels (homonim/raster_pair.py:193-224). """
    src_smaller = src.res[0] * src.res[1] <= ref.res[0] * ref.res[1]
    proc_crs = ProcCrs(proc_crs)
    if proc_crs == ProcCrs.auto:
        return ProcCrs.ref if src_smaller else ProcCrs.src
    if (proc_crs == ProcCrs.src and src_smaller) or (proc_crs == ProcCrs.ref and not src_smaller):
        import warnings
        rec = ProcCrs.ref if src_smaller else ProcCrs.src
        warnings.warn(f'proc_crs={rec} is recommended for these pixel sizes.', category=ConfigWarning)
    return proc_crs


def block_pairs_multires(src: Grid, ref: Grid, proc_crs: ProcCrs, n_bands: int, overlap: Tuple[int, int] = (0, 0),
                         max_block_mem: float = math.inf) -> Iterator[BlockPair]:
    """
    The reference's block partition for a source / reference pair on DIFFERENT grids of one CRS
    (homonim/raster_pair.py:227-269,342-428): blocks are cut on the processing grid, then mapped to whole-pixel windows
    of the other grid (in-blocks expanded, out-blocks rounded).  Source in-blocks may reach beyond the image (boundless).
    """
    src_win, ref_win = pair_windows(src, ref)
    proc_is_ref = ProcCrs(proc_crs) == ProcCrs.ref
    proc, other = (ref, src) if proc_is_ref else (src, ref)
    proc_win = ref_win if proc_is_ref else src_win
    src_area, ref_area = src.res[0] * src.res[1], ref.res[0] * ref.res[1]
    if proc_is_ref:
        mem_scale = src_area / ref_area if ref_area > src_area else 1.
    else:
        mem_scale = 1. if ref_area > src_area else ref_area / src_area
    mem = math.inf if (max_block_mem is None or max_block_mem <= 0) else max_block_mem * mem_scale
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', ConfigWarning)  # the small-block warning is re-issued below in source pixels
        blk_r, blk_c = auto_block_shape((proc_win.height, proc_win.width), mem)
    if (blk_r / mem_scale < 256 or blk_c / mem_scale < 256) and (blk_r < proc_win.height or blk_c < proc_win.width):
        warnings.warn(f'The auto block shape is small: {(blk_r, blk_c)}.  Increase `max_block_mem` to improve '
                      'processing times.', category=ConfigWarning)
    ov_r, ov_c = int(overlap[0]), int(overlap[1])
    if blk_r <= ov_r or blk_c <= ov_c:
        raise BlockSizeError('The auto block shape is smaller than the overlap.  Increase `max_block_mem`.')
    p_r0, p_c0 = proc_win.row_off, proc_win.col_off
    p_r1, p_c1 = p_r0 + proc_win.height, p_c0 + proc_win.width
    for band_i in range(n_bands):
        for r in range(p_r0 - ov_r, p_r1 - ov_r, blk_r):
            for c in range(p_c0 - ov_c, p_c1 - ov_c, blk_c):
                in_r0, in_c0 = max(r, p_r0), max(c, p_c0)
                in_r1, in_c1 = min(r + blk_r + 2 * ov_r, p_r1), min(c + blk_c + 2 * ov_c, p_c1)
                out_r0, out_c0 = max(r + ov_r, p_r0), max(c + ov_c, p_c0)
                out_r1, out_c1 = min(r + blk_r + ov_r, p_r1), min(c + blk_c + ov_c, p_c1)
                outer = in_r0 <= p_r0 or in_c0 <= p_c0 or in_r1 >= p_r1 or in_c1 >= p_c1
                proc_in = Window(in_c0, in_r0, in_c1 - in_c0, in_r1 - in_r0)
                proc_out = Window(out_c0, out_r0, out_c1 - out_c0, out_r1 - out_r0)
                other_in = expand_window_to_grid(other.window(*proc.window_bounds(proc_in)))
                other_out = round_window_to_grid(other.window(*proc.window_bounds(proc_out)))
                if proc_is_ref:
                    yield BlockPair(band_i, other_in, proc_in, other_out, proc_out, outer)
                else:
                    yield BlockPair(band_i, proc_in, other_in, proc_out, other_out, outer)


def _as_affine(transform, name: str) -> Optional[Affine]:
    if transform is None or isinstance(transform, Affine):
        return transform
    try:
        vals = [float(v) for v in transform]
    except TypeError:
        raise ValueError(f'`{name}` must be an Affine or a sequence of its six coefficients') from None
    if len(vals) not in (6, 9):
        raise ValueError(f'`{name}` must be an Affine or a sequence of its six coefficients')
    return Affine(*vals[:6])


def north_up(array: np.ndarray, transform: Optional[Affine]):
    """ (array, transform) with rows running north to south and columns west to east: a raster whose geo-transform has a
    positive row step (south-up) or a negative column step is flipped along that axis -- what the reference's
    ``utils.same_orientation_crs`` obtains by re-projecting it through a WarpedVRT.  A flip cannot bring a rotated or sheared
    grid north-up: ``RasterFuse`` warps those on the device (``_north_up_warp``), this function refuses them. """
    if transform is None:
        return array, transform
    if transform.b or transform.d:
        raise NotImplementedError('rotated / sheared rasters are not built (GDAL warp)')
    a, b, c, d, e, f = transform[:6]
    if e > 0:
        array = np.ascontiguousarray(array[..., ::-1, :])
        f, e = f + e * array.shape[-2], -e
    if a < 0:
        array = np.ascontiguousarray(array[..., ::-1])
        c, a = c + a * array.shape[-1], -a
    return array, Affine(a, b, c, d, e, f)


def dataset_masked(tif):
    """ A raster ``tiff.read_tiff`` returned as the reference reads it (``RasterArray.from_rio_dataset``, homonim/raster_array.py:
    161-197): -> (array, nodata, descriptions) without the alpha bands and, where the dataset has a mask, as float32 with NaN
    wherever it is false -- every band alike.  The rule: an internal mask masks the image and the nodata tag is
    ignored; otherwise the nodata tag stands; otherwise the trailing alpha band of a 2- or 4-band uint8 / uint16 file masks it
    (``tif.mask_band``), valid where it is not 0; otherwise every pixel is valid.  The mask is applied by
    ``Context.dataset_mask`` of the process-wide context.  A file without mask or alpha band comes back as it is. """
    if tif.mask is None and not tif.alpha_bands:
        return tif.array, tif.nodata, tif.descriptions
    keep = [b for b in range(tif.array.shape[0]) if b not in tif.alpha_bands]
    if not keep:
        raise ValueError('the raster has alpha bands only')
    # (alpha bands usually trail: the bands that stay are then a view of the file's array)
    bands = tif.array if not tif.alpha_bands else tif.array[:len(keep)] if keep == list(range(len(keep))) else tif.array[keep]
    descriptions = tuple(tif.descriptions[b] for b in keep) if len(tif.descriptions) == tif.array.shape[0] else tif.descriptions
    if tif.mask is not None:
        return _hk.default_context().dataset_mask(bands, mask=tif.mask), float('nan'), descriptions
    if tif.mask_band is not None:
        return _hk.default_context().dataset_mask(bands, alpha=tif.array[tif.mask_band]), float('nan'), descriptions
    return bands, tif.nodata, descriptions


def shard(items: Sequence, index: int, count: int, contiguous: bool = False) -> List:
    """ The work items of shard ``index`` of ``count``: round-robin, or -- ``contiguous`` -- consecutive runs of (almost)
    equal length, which keeps a shard inside as few bands as possible (the block list is band-major,
    homonim/raster_pair.py:381-389).  Either way the shards are disjoint and cover ``items``. """
    if count < 1 or not (0 <= index < count):
        raise ValueError(f'bad shard {index} of {count}')
    if contiguous:
        n = len(items)
        return list(items[index * n // count:(index + 1) * n // count])
    return list(items[index::count])


class BlockCall(NamedTuple):
    """ Consecutive bands of one spatial block: one device-resident call (``group_block_calls``). """
    band_i: int            # the first band
    n_bands: int
    src_in_block: Window
    ref_in_block: Window
    src_out_block: Window
    ref_out_block: Window

    @property
    def bands(self) -> range:
        return range(self.band_i, self.band_i + self.n_bands)


def group_block_calls(blocks: Sequence[BlockPair]) -> List[BlockCall]:
    """ The calls of the resident block loop for a (shard of a) block list: the pairs that share their four windows form a group,
    in the order in which the list first names the windows, and every maximal run of consecutive band indices of a group is one
    call.  A whole block list gives one call per spatial block for all bands; a shard gives the runs that it holds.  A pure
    function of the list: every (band, block) pair of it is in exactly one call. """
    groups: Dict[Tuple[Window, Window, Window, Window], List[int]] = {}
    for bp in blocks:
        groups.setdefault((bp.src_in_block, bp.ref_in_block, bp.src_out_block, bp.ref_out_block), []).append(bp.band_i)
    calls = []
    for windows, bands in groups.items():
        bands = sorted(set(bands))
        start = 0
        for i in range(1, len(bands) + 1):
            if i == len(bands) or bands[i] != bands[i - 1] + 1:
                calls.append(BlockCall(bands[start], i - start, *windows))
                start = i
    return calls


def _is_path(x) -> bool:
    return isinstance(x, (str, os.PathLike))


def default_devices(devices: Optional[Sequence[int]] = None) -> Sequence[int]:
    """ The ``devices`` of a device configuration; None: the one device of this process -- HOMONIM_AMD_DEVICE, else the launcher's
    LOCAL_RANK, else 0. """
    if devices is None:
        return [int(os.environ.get('HOMONIM_AMD_DEVICE', os.environ.get('LOCAL_RANK', '0')))]
    return devices


class RasterFuse:
    """
    Correct a source raster to surface reflectance by fusion with a reference raster.

    src, ref : float32 arrays (bands, height, width) or (height, width), ``RasterArray`` instances, or GeoTIFF paths
    (nodata, CRS and geo-transform then come from the files; bands are paired in file order, alpha bands left out; a file with
    an internal mask, or with an alpha band and no nodata tag, is read as float32 with NaN outside its mask: ``dataset_masked``.
    A masked uint8 raster so occupies four times its file size on the host, as it does in the reference).
    The other constructor arguments mirror homonim.RasterFuse / RasterPairReader where they make sense in memory.
    """

    create_model_config = staticmethod(KernelModel.create_config)

    def __init__(self, src: Union[np.ndarray, RasterArray], ref: Union[np.ndarray, RasterArray],
                 src_nodata: Optional[float] = float('nan'), ref_nodata: Optional[float] = float('nan'),
                 proc_crs: ProcCrs = ProcCrs.auto, crs: Optional[CRS] = None, transform: Optional[Affine] = None,
                 ref_transform: Optional[Affine] = None, ref_crs: Optional[CRS] = None, inflate: str = 'host'):
        """
        ``inflate``: who inflates the DEFLATE blocks of ``src`` / ``ref`` given as GeoTIFF paths: 'host' (default) -- zlib on
        this thread, as ever; 'device' -- ``Context.inflate_image`` of the process-wide context: the same pixels.  LZW blocks go
        to the library's host decoder (``_hk.lzw_image_host``) under 'host' and to ``Context.lzw_image`` under 'device'.
        ``transform`` / ``ref_transform``: geo-transforms of the source / reference rasters (north-up).  When they (or the
        shapes) differ, blocks are cut on the processing grid and re-sampled on the device as the reference does through
        GDAL (RefSpaceModel / SrcSpaceModel); the reference must cover the source.  ``crs`` / ``ref_crs``: their CRSs (taken
        from files and ``RasterArray`` instances); ``ref_crs`` defaults to ``crs``.  When the two differ the processing-grid
        image -- ``proc_crs=src``: the source, otherwise the reference -- is first warped into the other's CRS
        (``_to_one_crs``), with the reference's warning.
        """
        decoders = _hk.block_decoders(inflate, _hk.default_context if (_is_path(src) or _is_path(ref)) else None)
        src, src_nodata, crs, transform, self._src_filename, _ = self._open(src, src_nodata, crs, transform, decoders)
        # (the band descriptions of a reference opened from a file name the parameter bands)
        ref, ref_nodata, ref_crs, ref_transform, self._ref_filename, self._ref_descriptions = self._open(
            ref, ref_nodata, ref_crs, ref_transform, decoders)
        if src.ndim != 3 or ref.ndim != 3:
            raise ValueError('`src` and `ref` must be 2-D or 3-D (bands first) arrays')
        # transforms may come as plain 6-tuples (a, b, c, d, e, f)
        transform = _as_affine(transform, 'transform')
        ref_transform = _as_affine(ref_transform, 'ref_transform')
        # south-up (or column-mirrored) rasters are brought to north-up first, as the reference does through a WarpedVRT
        # (homonim/utils.py:190-209; for an axis-aligned raster that re-projection is the flip); outputs are north-up.  Rotated and
        # sheared rasters are left for the warps below: the same WarpedVRT, bilinear
        src_rotated = transform is not None and is_rotated(transform)
        ref_rotated = ref_transform is not None and is_rotated(ref_transform)
        if not src_rotated:
            src, transform = north_up(src, transform)
        if not ref_rotated:
            ref, ref_transform = north_up(ref, ref_transform)
        if ref.shape[0] < src.shape[0]:
            raise ValueError('`ref` has fewer bands than `src`')
        if crs is not None and ref_crs is not None and not crs_defs.same_crs(crs, ref_crs):
            src, src_nodata, crs, transform, ref, ref_nodata, ref_transform, proc_crs = self._to_one_crs(
                src, src_nodata, crs, transform, ref, ref_nodata, ref_crs, ref_transform, ProcCrs(proc_crs))
        else:
            if src_rotated:
                src, src_nodata, transform = self._north_up_warp(src, src_nodata, crs or ref_crs, transform)
            if ref_rotated:
                ref, ref_nodata, ref_transform = self._north_up_warp(ref, ref_nodata, ref_crs or crs, ref_transform)
        self._src, self._ref = src, ref
        self._src_nodata, self._ref_nodata = src_nodata, ref_nodata
        self._crs = crs or CRS()
        self._transform = transform or Affine.identity()
        self._ref_transform = ref_transform or self._transform
        self._src_grid = Grid(self._transform, *src.shape[-2:])
        self._ref_grid = Grid(self._ref_transform, *ref.shape[-2:])
        self._same_grid = self._src_grid == self._ref_grid
        if not self._same_grid:
            l, b, r, t = self._src_grid.bounds
            rl, rb, rr, rt = self._ref_grid.bounds
            if l < rl or r > rr or b < rb or t > rt:  # homonim/raster_pair.py:93-94
                from homonim_amd.errors import ImageContentError
                raise ImageContentError('Reference extent does not cover source image')
        # auto resolves to the grid with the larger pixels, the reference grid on ties (homonim/raster_pair.py:193-224)
        self._proc_crs = resolve_proc_crs(self._src_grid, self._ref_grid, proc_crs)
        self._closed = False
        self._write_lock = threading.Lock()

    @staticmethod
    def _open(x, nodata, crs, transform, decoders):
        """ ``x`` -- a GeoTIFF path, a ``RasterArray`` or an array -- with the caller's nodata, CRS and geo-transform, which a file or
        a ``RasterArray`` replaces by its own -> (array, nodata, crs, transform, filename, descriptions), a 2-D array made 3-D. """
        filename, descriptions = None, ()
        if _is_path(x):  # a GeoTIFF, as homonim.RasterFuse(src_filename, ref_filename, ...)
            from homonim_amd.tiff import read_tiff
            filename = os.fspath(x)
            tif = read_tiff(x, inflater=decoders[0], lzw=decoders[1])
            x, nodata, descriptions = dataset_masked(tif)
            crs, transform = tif.crs, tif.transform
        if isinstance(x, RasterArray):
            x, nodata, crs, transform = x.array, x.nodata, x.crs, x.transform
        x = np.asarray(x)
        return (x[None] if x.ndim == 2 else x), nodata, crs, transform, filename, descriptions

    @staticmethod
    def _device_context():
        return _hk.get_context(default_devices()[0])

    @classmethod
    def _north_up_warp(cls, array, nodata, crs, transform):
        """ A rotated / sheared raster brought north-up in its own CRS, whatever its label: warped bilinearly onto
        ``geo.suggested_warp_grid`` of that CRS, all bands in one device call (homonim/utils.py:190-209).  Returns (array, nodata,
        transform); an image without nodata gets NaN for what the warp leaves empty. """
        crs = crs or CRS()
        out_nodata = float('nan') if nodata is None else nodata
        grid, shape = suggested_warp_grid(crs, transform, array.shape[-2:], crs)
        ra = RasterArray(array, crs, transform, nodata=nodata).reproject(
            transform=grid, shape=shape, nodata=out_nodata, resampling=Resampling.bilinear, context=cls._device_context())
        return ra.array, out_nodata, ra.transform

    def _to_one_crs(self, src, src_nodata, crs, transform, ref, ref_nodata, ref_crs, ref_transform, proc_crs: ProcCrs):
        """ Source and reference in different CRSs: what ``RasterPairReader`` does with such a pair (homonim/raster_pair.py:160-166,
        homonim/utils.py:190-209).  Warn; resolve ``proc_crs=auto`` from the pixel areas, the reference's pixel brought into the
        source's CRS at the source's centre; warp the processing-grid image -- ``proc_crs=src``: the source, otherwise the reference
        -- into the other's CRS on ``geo.suggested_warp_grid``, bilinear, all bands in one device call.  Returns the pair on one
        CRS and the resolved ``proc_crs``; an image without nodata gets NaN for what the warp leaves empty.
        Rotated / sheared grids: pixel sizes are the lengths of the column and row step vectors, the source's centre goes through
        the full affine; the processing-grid image goes from its rotated grid into the other CRS in that single warp, the other
        image, if rotated, is brought north-up in its own CRS (``_north_up_warp``). """
        import warnings
        names = [os.path.basename(fn) if fn else 'memory' for fn in (self._src_filename, self._ref_filename)]
        warnings.warn(f'Source and reference image will be re-projected to the same CRS: {names[0]} and {names[1]}',
                      category=ImageFormatWarning)
        crs_defs.definitions(crs, ref_crs)   # NotImplementedError naming an unknown CRS / two ellipsoids
        if transform is None or ref_transform is None:
            raise ValueError('source and reference in different CRSs need their geo-transforms (`transform`, `ref_transform`)')
        # the reference's pixel at the source's centre, in source CRS units
        h, w = src.shape[-2:]
        xc, yc = transform * (w / 2, h / 2)   # (the axis-aligned c + a * w / 2, f + e * h / 2 to the bit: b = d = 0)
        xr, yr = crs_defs.transform_coords(crs, ref_crs, xc, yc)
        px, py = crs_defs.transform_coords(ref_crs, crs, xr + np.array([0., ref_transform.a, ref_transform.b]),
                                           yr + np.array([0., ref_transform.d, ref_transform.e]))
        ref_res = (float(np.hypot(px[1] - px[0], py[1] - py[0])), float(np.hypot(px[2] - px[0], py[2] - py[0])))
        if not all(math.isfinite(v) and v > 0 for v in ref_res):
            from homonim_amd.errors import ImageContentError
            raise ImageContentError('Reference extent does not cover source image')
        src_res = pixel_size(transform)   # (abs(a), abs(e)) exactly for an axis-aligned grid
        proc_crs = resolve_proc_crs(Grid(Affine(src_res[0], 0., 0., 0., -src_res[1], 0.), h, w),
                                    Grid(Affine(ref_res[0], 0., 0., 0., -ref_res[1], 0.), 1, 1), proc_crs)
        ctx = self._device_context()
        # the image that stays in its CRS, if rotated, goes north-up there
        if proc_crs == ProcCrs.src and is_rotated(ref_transform):
            ref, ref_nodata, ref_transform = self._north_up_warp(ref, ref_nodata, ref_crs, ref_transform)
        elif proc_crs != ProcCrs.src and is_rotated(transform):
            src, src_nodata, transform = self._north_up_warp(src, src_nodata, crs, transform)
        if proc_crs == ProcCrs.src:
            nodata = float('nan') if src_nodata is None else src_nodata
            ra = RasterArray(src, crs, transform, nodata=src_nodata).reproject(crs=ref_crs, nodata=nodata,
                                                                              resampling=Resampling.bilinear, context=ctx)
            src, src_nodata, crs, transform = ra.array, nodata, ref_crs, ra.transform
        else:
            nodata = float('nan') if ref_nodata is None else ref_nodata
            ra = RasterArray(ref, ref_crs, ref_transform, nodata=ref_nodata).reproject(crs=crs, nodata=nodata,
                                                                                      resampling=Resampling.bilinear, context=ctx)
            ref, ref_nodata, ref_transform = ra.array, nodata, ra.transform
        return src, src_nodata, crs, transform, ref, ref_nodata, ref_transform, proc_crs

    # -- context manager parity with the reference (files there, nothing to open here) --------------------------------
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._closed = True

    @property
    def proc_crs(self) -> ProcCrs:
        return self._proc_crs

    @property
    def src_bands(self) -> Tuple[int, ...]:
        return tuple(range(1, self._src.shape[0] + 1))

    @property
    def shape(self) -> Tuple[int, int]:
        return tuple(self._src.shape[-2:])

    # -- configuration factories (homonim/fuse.py:89-149) -------------------------------------------------------------
    @staticmethod
    def create_block_config(threads: int = 0, max_block_mem: float = 100) -> Dict:
        return dict(threads=utils.validate_threads(threads), max_block_mem=max_block_mem)

    @staticmethod
    def create_out_profile(driver: str = 'GTiff', dtype: str = RasterArray.default_dtype,
                           nodata: Optional[float] = RasterArray.default_nodata,
                           creation_options: Optional[Dict] = None) -> Dict:
        creation_options = creation_options or dict(
            tiled=True, blockxsize=512, blockysize=512, compress='deflate', interleave='band',
            photometric='minisblack', bigtiff='if_safer'
        )
        return dict(driver=driver, dtype=dtype, nodata=nodata, creation_options=creation_options)

    @staticmethod
    def create_device_config(devices: Optional[Sequence[int]] = None, streams: int = 4, rank: int = 0,
                             world_size: int = 1, contiguous: bool = False, pin: bool = True,
                             separate_contexts: bool = False, deflate: str = 'host', resident: bool = False) -> Dict:
        """ (this package only) GPUs of this process, streams per GPU, this process's shard of the block list
        (round-robin, or ``contiguous`` runs), whether every entry of ``devices`` gets a context of its own even when a
        device is listed twice, and ``pin``: True (default) -- the rasters are registered in place for the duration of the
        block loop (``hk_host_register``) and copied directly: 10-17 % more end-to-end throughput than through the staging
        ring (profiles/r04_streamed_host.txt); a raster that cannot be registered (``ulimit -l``, foreign memory) and every
        array the library did not page-lock itself travel through the library's own page-locked staging ring, so the runtime
        is never handed pageable memory either way (the registered path ran clean as the first process of five fresh
        leases, profiles/r04_abort_followup.txt); False -- everything through the staging ring: the GPU never touches
        caller-allocated pages.  ``deflate``: who compresses the tiles of the GeoTIFFs ``process`` writes: 'host' (default) --
        zlib level 6 on the writing thread, byte for byte as before; 'device' -- ``Context.deflate_tiles``: the same pixels, tags
        and overviews in files a few percent larger, written without the minutes of host zlib.  ``resident``: where
        the rasters of a source / reference pair on DIFFERENT grids live during ``process``: False (default) -- on the host, every
        block pair staged up and down band by band, as ever; True -- on the device: source and reference go up once, every block
        pair runs on the resident rasters all bands at a time (``fit_apply_dev`` of the model), overviews are built there and
        the results come down once: the same bytes in arrays and files.  ``process`` then refuses, before anything
        is allocated or launched, a pair on a shared grid, more than one device or ``separate_contexts``, an in-block taller than
        65535 rows and rasters that do not fit the device's free memory; it never falls back to the host path.  Read by
        ``RasterFuse.process`` only. """
        if deflate not in ('host', 'device'):
            raise ValueError(f"`deflate` must be 'host' or 'device', not {deflate!r}")
        return dict(devices=None if devices is None else list(devices), streams=int(streams), rank=int(rank),
                    world_size=int(world_size), contiguous=bool(contiguous), pin=bool(pin),
                    separate_contexts=bool(separate_contexts), deflate=deflate, resident=bool(resident))

    def block_pairs(self, overlap: Tuple[int, int] = (0, 0), max_block_mem: float = math.inf) -> Iterable[BlockPair]:
        if self._same_grid:
            return block_pairs(self.shape, self._src.shape[0], overlap, max_block_mem)
        return block_pairs_multires(self._src_grid, self._ref_grid, self._proc_crs, self._src.shape[0], overlap,
                                    max_block_mem)

    @staticmethod
    def _read_boundless(band: np.ndarray, nodata: Optional[float], win: Window) -> Tuple[np.ndarray, Optional[float]]:
        """ A window of a band that may reach beyond it, filled with nodata outside (RasterArray.from_rio_dataset,
        homonim/raster_array.py:172-188: NaN when the raster has no nodata value). """
        h, w = band.shape
        r0, c0 = max(win.row_off, 0), max(win.col_off, 0)
        r1, c1 = min(win.row_off + win.height, h), min(win.col_off + win.width, w)
        inside = r0 == win.row_off and c0 == win.col_off and r1 == win.row_off + win.height and c1 == win.col_off + win.width
        if inside:
            return band[r0:r1, c0:c1], nodata
        fill = float('nan') if nodata is None else nodata
        dtype = np.float32 if (nodata is None or (isinstance(fill, float) and math.isnan(fill))) else band.dtype
        out = np.full((win.height, win.width), fill, dtype=dtype)
        if r1 > r0 and c1 > c0:
            out[r0 - win.row_off:r1 - win.row_off, c0 - win.col_off:c1 - win.col_off] = band[r0:r1, c0:c1]
        return out, fill

    # -- the block loop -----------------------------------------------------------------------------------------------
    @property
    def _param_grid(self) -> Grid:
        """ parameters live on the processing grid (homonim/fuse.py:254-293): the reference's when proc_crs == ref """
        return self._ref_grid if (self._proc_crs == ProcCrs.ref and not self._same_grid) else self._src_grid

    def _band_params(self, params: np.ndarray, band_i: int) -> np.ndarray:
        """ the planes of band ``band_i`` in the parameter raster: parameter ``pi`` of band ``b`` is plane ``pi * n_src + b``, the band
        order of the reference's parameter file (fuse.py:316) """
        return params[band_i::self._src.shape[0]]

    def _read_pair(self, bp: BlockPair) -> Tuple[RasterArray, RasterArray]:
        """ the in-blocks of a pair in the rasters' own dtypes (boundless: a source in-block may reach beyond the image), their
        transforms translated to the blocks (homonim/fuse.py:304) """
        s_arr, s_nd = self._read_boundless(self._src[bp.band_i], self._src_nodata, bp.src_in_block)
        r_arr, r_nd = self._read_boundless(self._ref[bp.band_i], self._ref_nodata, bp.ref_in_block)
        src_tf = self._transform * Affine.translation(bp.src_in_block.col_off, bp.src_in_block.row_off)
        ref_tf = self._ref_transform * Affine.translation(bp.ref_in_block.col_off, bp.ref_in_block.row_off)
        return RasterArray(s_arr, self._crs, src_tf, nodata=s_nd), RasterArray(r_arr, self._crs, ref_tf, nodata=r_nd)

    @staticmethod
    def _crop(bp: BlockPair) -> Tuple[slice, slice]:
        """ slices of the out-block inside the in-block (the halo crop of homonim/raster_array.py:478-491) """
        r0 = bp.src_out_block.row_off - bp.src_in_block.row_off
        c0 = bp.src_out_block.col_off - bp.src_in_block.col_off
        return slice(r0, r0 + bp.src_out_block.height), slice(c0, c0 + bp.src_out_block.width)

    @staticmethod
    def _put(dst_plane: np.ndarray, block_arr: np.ndarray, in_win: Window, out_win: Window):
        """ the out-block of a block read at ``in_win`` into a plane of an output raster, clipped to the plane (inside it: the
        halo crop, ``dst_plane[out_win] = block_arr[_crop]``) """
        h, w = dst_plane.shape
        r0, c0 = max(out_win.row_off, 0), max(out_win.col_off, 0)
        r1, c1 = min(out_win.row_off + out_win.height, h), min(out_win.col_off + out_win.width, w)
        if r1 > r0 and c1 > c0:
            dst_plane[r0:r1, c0:c1] = block_arr[r0 - in_win.row_off:r1 - in_win.row_off,
                                                c0 - in_win.col_off:c1 - in_win.col_off]

    def _process_block(self, bp: BlockPair, model: KernelModel, corr: np.ndarray, params: Optional[np.ndarray],
                       out_nodata: Optional[float], valid: Optional[np.ndarray] = None):
        """ read -> fit + apply (+ output dtype conversion) on the GPU -> write the out-block (homonim/fuse.py:295-319): fused into one
        kernel on a shared grid, across grids with RefSpaceModel / SrcSpaceModel doing the re-sampling on the device.  ``valid``: the
        (H, W) validity raster, which the blocks of band 0 fill where they fill ``corr[0]`` """
        src_ra, ref_ra = self._read_pair(bp)
        band_params = self._band_params(params, bp.band_i) if params is not None else None
        if bp.band_i != 0:
            valid = None
        if model.fuses_into(src_ra, ref_ra):
            # the out-block goes straight from the device into the corrected / parameter rasters (no block-sized
            # temporaries, no host-side crop copy; asynchronous when the rasters are page-locked)
            rs, cs = bp.src_out_block.toslices()
            crop = self._crop(bp)
            window = (crop[0].start, crop[1].start, bp.src_out_block.height, bp.src_out_block.width)
            model.fit_apply_into(src_ra, ref_ra, window, corr[bp.band_i][rs, cs],
                                 band_params[:, rs, cs] if params is not None else None, out_nodata=out_nodata,
                                 valid_dst=valid[rs, cs] if valid is not None else None)
            return
        # one upload / download per block in the rasters' own dtypes, everything else stays in HBM (RefSpaceModel and
        # SrcSpaceModel alike: hk_refspace_fit_apply, hk_srcspace_fit_apply)
        corr_ra, param_ra, *block_valid = model.fit_apply(src_ra, ref_ra, want_params=params is not None, out_dtype=corr.dtype.name,
                                                          out_nodata=out_nodata, want_valid=valid is not None)
        self._put(corr[bp.band_i], corr_ra.array, bp.src_in_block, bp.src_out_block)
        if valid is not None:
            self._put(valid, block_valid[0], bp.src_in_block, bp.src_out_block)
        if params is not None:
            p_in, p_out = (bp.ref_in_block, bp.ref_out_block) if self._param_grid is self._ref_grid else \
                (bp.src_in_block, bp.src_out_block)
            for plane, block in zip(band_params, param_ra.array):
                self._put(plane, block, p_in, p_out)

    def process(self, corr_filename: Optional[Union[str, os.PathLike]] = None, model: Model = KernelModel.default_model,
                kernel_shape: Tuple[int, int] = KernelModel.default_kernel_shape,
                param_filename: Optional[Union[str, os.PathLike, bool]] = None, build_ovw: bool = True,
                overwrite: bool = False, model_config: Optional[Dict] = None, out_profile: Optional[Dict] = None,
                block_config: Optional[Dict] = None, device_config: Optional[Dict] = None,
                corr_out: Optional[np.ndarray] = None, return_valid: bool = False):
        """
        Same arguments as homonim.RasterFuse.process (fuse.py:321-332) plus ``device_config``.  Returns
        ``(corrected, params)``: float32 arrays (bands, H, W) and (n_param_bands * bands, H, W) or None.  When
        ``corr_filename`` / ``param_filename`` are paths the arrays are also written there: ``.tif`` as a tiled DEFLATE
        GeoTIFF with the reference's FUSE_* provenance tags (homonim_amd/tiff.py), anything else with ``numpy.save``.
        ``out_profile['creation_options']`` shape both ``.tif`` files: ``compress`` ('deflate', or None / 'none'), ``predictor``
        (1, 2 or 3), ``blockxsize`` = ``blockysize`` (a multiple of 16 in 16..512), ``bigtiff`` ('yes', 'no', 'if_needed',
        'if_safer': ``tiff.bigtiff_wanted``), ``tiled`` (True) and ``interleave`` ('band'); a key that is missing takes the
        default profile's value, a value that cannot be written is a ``ValueError`` naming the key before any block is
        processed, and ``driver``, ``photometric`` and every other key are accepted and ignored.  With no ``.tif`` to write
        (arrays only, ``.npy``) all of them are ignored as before.  One profile shapes both files and the parameter file is
        float32 whatever the output dtype, so the predictor is checked against each ``.tif`` that is written: an integer
        corrected ``.tif`` beside a parameter ``.tif`` leaves predictor 1 only.  ``build_ovw`` (default, as in the reference:
        fuse.py:152-165): a ``.tif`` gets internal overviews -- ``overview_factors(shape)``: factors 2, 4, ... while the shorter
        side keeps 256 pixels, ``Resampling.average`` cascaded level to level, built on the GPU (``Context.overviews``) from the
        finished rasters under their own dtype and nodata; a raster too small for a level, ``build_ovw=False`` and ``.npy``
        outputs give the file without them.  The returned arrays are the same either way.
        With ``world_size > 1`` only this rank's blocks are filled in (others stay nodata).
        ``corr_out``: a caller-owned corrected raster (bands, H, W) of the output dtype to fill instead of a new one, e.g.
        page-locked memory of a pipeline that processes many rasters (it is NOT pre-filled with nodata).
        An output WITHOUT a nodata value (``out_profile['nodata'] is None``) written to a ``.tif`` gets an internal mask, as the
        reference's does (``rio_dataset.write_mask`` "once (for first band) if nodata is None", raster_array.py:493-500, under
        ``GDAL_TIFF_INTERNAL_MASK=True``, raster_pair.py:303): a 1-bit mask directory behind the main image (``tiff.write_tiff``), and
        the overviews are averaged under that mask and carry masks of their own.  The mask is the validity of the corrected block
        BEFORE its conversion to the output dtype -- a pixel is valid where its float32 corrected value is not NaN -- gathered on the
        device next to the conversion, and THE FILE'S MASK IS BAND 1'S: one (H, W) uint8 raster, zero-filled, that only the blocks of
        the first band fill (255 / 0), placed like ``corr[0]``; with ``world_size > 1`` it holds this rank's blocks only.
        ``return_valid=True`` returns ``(corrected, params, valid)`` with that raster, whatever the nodata and the file type
        (``.npy`` outputs write no mask: this is the way to get it); otherwise, and with a nodata value, nothing is gathered.
        The parameter file has nodata NaN and never a mask.
        """
        if self._closed:
            raise IoError('The raster pair has been closed')
        model_type = Model(model)
        overlap = utils.overlap_for_kernel(kernel_shape)
        model_config = RasterFuse.create_model_config(**(model_config or {}))
        block_config = RasterFuse.create_block_config(**(block_config or {}))
        out_profile = RasterFuse.create_out_profile(**(out_profile or {}))
        device_config = RasterFuse.create_device_config(**(device_config or {}))
        want_params = param_filename is not None and param_filename is not False
        if device_config['resident']:
            self._check_resident(device_config)
        out_dtype, nodata, write_options = self._resolve_output(corr_filename, param_filename, want_params, overwrite, out_profile)
        models, own_contexts = self._build_models(model_type, kernel_shape, want_params, model_config, device_config)
        n_param = models[0].n_param
        if device_config['resident']:
            return self._process_resident(corr_filename, param_filename, want_params, build_ovw, models[0], model_type, kernel_shape,
                                          model_config, block_config, device_config, out_dtype, nodata, write_options, corr_out,
                                          return_valid)
        corr, params = self._allocate(out_dtype, nodata, corr_out, n_param if want_params else 0)
        write_mask = nodata is None and self._is_tiff(corr_filename)
        valid = np.zeros(self.shape, np.uint8) if (return_valid or write_mask) else None
        blocks = list(self.block_pairs(overlap=overlap, max_block_mem=block_config['max_block_mem']))
        blocks = shard(blocks, device_config['rank'], device_config['world_size'], device_config['contiguous'])
        want_ovw = (build_ovw and self._is_tiff(corr_filename), build_ovw and want_params and self._is_tiff(param_filename))
        overviews = self._run(blocks, models, own_contexts, corr, params, nodata, block_config['threads'], device_config['pin'],
                              want_ovw, valid, write_mask)
        compressor = models[0].context.deflate_tiles if device_config['deflate'] == 'device' else None
        self._write(corr_filename, param_filename if want_params else None, corr, params, nodata, n_param, overviews,
                    dict(model=model_type, kernel_shape=tuple(kernel_shape), **model_config), compressor, write_options,
                    valid if write_mask else None)
        return (corr, params, valid) if return_valid else (corr, params)

    def _process_resident(self, corr_filename, param_filename, want_params: bool, build_ovw: bool, model: KernelModel, model_type: Model,
                          kernel_shape, model_config: Dict, block_config: Dict, device_config: Dict, out_dtype: np.dtype, nodata,
                          write_options: Optional[Dict], corr_out: Optional[np.ndarray], return_valid: bool):
        """ ``process`` with ``resident=True``: the same block list and shard, the same files and return values; the rasters live on
        the device from the first block to the last (homonim_amd/resident.py). """
        from homonim_amd.resident import ResidentRun
        n_param = model.n_param
        write_mask = nodata is None and self._is_tiff(corr_filename)
        blocks = list(self.block_pairs(overlap=utils.overlap_for_kernel(kernel_shape), max_block_mem=block_config['max_block_mem']))
        blocks = shard(blocks, device_config['rank'], device_config['world_size'], device_config['contiguous'])
        want_ovw = (build_ovw and self._is_tiff(corr_filename), build_ovw and want_params and self._is_tiff(param_filename))
        corr, params, valid, overviews = ResidentRun(
            self, model, group_block_calls(blocks), out_dtype, nodata, corr_out, n_param if want_params else 0,
            return_valid or write_mask, block_config['threads'], device_config['streams'], device_config['pin'], want_ovw,
            write_mask).run()
        compressor = model.context.deflate_tiles if device_config['deflate'] == 'device' else None
        self._write(corr_filename, param_filename if want_params else None, corr, params, nodata, n_param, overviews,
                    dict(model=model_type, kernel_shape=tuple(kernel_shape), **model_config), compressor, write_options,
                    valid if write_mask else None)
        return (corr, params, valid) if return_valid else (corr, params)

    def _check_resident(self, device_config: Dict):
        """ What ``resident=True`` refuses from the pair and the device configuration alone, before any library call """
        if self._same_grid:
            raise ValueError('`resident=True` is for a source and a reference on different grids: on a shared grid the host path is '
                             'already one fused kernel per block (and SrcSpaceModel with mask_partial has no device-resident form there)')
        if len(default_devices(device_config['devices'])) != 1 or device_config['separate_contexts']:
            raise ValueError('`resident=True` takes one device and one context: the resident rasters live on one device '
                             f"(devices={device_config['devices']}, separate_contexts={device_config['separate_contexts']})")

    def _resolve_output(self, corr_filename, param_filename, want_params: bool, overwrite: bool, out_profile: Dict):
        """ -> (output dtype, output nodata, ``write_options`` or None) of a ``process`` call, which is refused here when a file exists
        and is not to be overwritten, or when the profile asks for what cannot be written. """
        for fn in (corr_filename, param_filename):
            if _is_path(fn) and os.path.exists(fn) and not overwrite:
                raise FileExistsError(f"Corrected / parameter file exists and won't be overwritten: {fn}")
        nodata = out_profile['nodata']
        out_dtype = np.dtype(out_profile['dtype'])
        if out_dtype.name not in _hk.DTYPE_CODES:
            raise ValueError(f"unsupported output dtype '{out_profile['dtype']}'")
        _hk.out_nodata_code(out_dtype, nodata)  # a nodata the dtype cannot hold is refused (homonim/raster_array.py:357-358)
        # the creation options shape .tif outputs only: with none to write they stay ignored
        tiff_dtypes = ([('the corrected file', out_dtype)] if self._is_tiff(corr_filename) else []) + \
                      ([('the parameter file', np.dtype(np.float32))] if want_params and self._is_tiff(param_filename) else [])
        return out_dtype, nodata, (self._write_options(out_profile['creation_options'], tiff_dtypes) if tiff_dtypes else None)

    def _build_models(self, model_type: Model, kernel_shape, want_params: bool, model_config: Dict, device_config: Dict):
        """ -> (models, own_contexts): one model with its context per entry of ``devices``; ``own_contexts``: those made for this
        call (``separate_contexts``), to be closed after it. """
        model_cls = SrcSpaceModel if self._proc_crs == ProcCrs.src else RefSpaceModel
        models, own_contexts, seen = [], [], set()
        for dev in default_devices(device_config['devices']):
            m = model_cls(model_type, kernel_shape, find_r2=want_params, **model_config)
            if device_config['separate_contexts'] and dev in seen:
                m.context = _hk.Context(dev, device_config['streams'])  # a second, independent context on this device
                own_contexts.append(m.context)
            else:
                m.context = _hk.get_context(dev, device_config['streams'])  # cached per process
            seen.add(dev)
            models.append(m)
        return models, own_contexts

    def _allocate(self, out_dtype: np.dtype, nodata, corr_out: Optional[np.ndarray], n_param: int):
        """ -> (corr, params): the corrected raster -- ``corr_out`` when given, else filled with nodata -- and the NaN-filled raster of
        ``n_param`` parameters per band on ``_param_grid``, None for ``n_param`` 0. """
        n_src = self._src.shape[0]
        if corr_out is not None:
            if corr_out.shape != (n_src, *self.shape) or corr_out.dtype != out_dtype or not corr_out.flags['C_CONTIGUOUS']:
                raise ValueError('`corr_out` must be a C-contiguous (bands, height, width) array of the output dtype')
            corr = corr_out
        else:
            fill = (np.nan if out_dtype.kind == 'f' else 0) if nodata is None else nodata
            corr = np.full((n_src, *self.shape), fill, dtype=out_dtype)
        grid = self._param_grid
        params = np.full((n_param * n_src, grid.height, grid.width), np.nan, dtype=np.float32) if n_param else None
        return corr, params

    def _run(self, blocks, models, own_contexts, corr, params, nodata, threads: int, pin: bool, want_ovw: Tuple[bool, bool],
             valid: Optional[np.ndarray] = None, masked_ovw: bool = False):
        """ The block loop -> (corr_ovw, param_ovw): the internal overviews asked for by ``want_ovw``, else None.  ``valid``: the
        validity raster the blocks of band 0 fill; ``masked_ovw``: the corrected raster's overviews are built under it, and
        corr_ovw is ``(levels, level_valids)``. """
        ctx = models[0].context
        # on request: page-lock the rasters in place for the duration of the block loop (direct copies); by default pageable
        # rasters go through the context's pinned staging ring (hk_api.hip stage_h2d / stage_d2h) block by block
        pinned = self._pin(ctx, [self._src, self._ref, corr, params, valid]) if pin else []
        try:
            self._run_blocks(blocks, lambda bp, wi: self._process_block(bp, models[wi], corr, params, nodata, valid),
                             [m.context for m in models], threads)
            # internal overviews of the files to be written, while the rasters are still page-locked (direct copies)
            return (self._overviews(ctx, corr, nodata, valid if masked_ovw else None) if want_ovw[0] else None,
                    self._overviews(ctx, params, float('nan')) if want_ovw[1] else None)
        finally:
            for arr in pinned:
                try:
                    ctx.unpin(arr)
                except Exception:
                    pass
            for c in own_contexts:
                c.close()

    def _write(self, corr_filename, param_filename, corr, params, nodata, n_param: int, overviews, settings: Dict, compressor,
               write_options: Optional[Dict], mask: Optional[np.ndarray] = None):
        """ The rasters into the files that are paths, with the provenance tags of homonim/fuse.py:193-207 (``settings``: model, kernel
        shape and model configuration of the run).  ``mask``: the internal mask of the corrected file; its overviews are then
        ``(levels, level_masks)``. """
        meta = dict(FUSE_SRC_FILE=os.path.basename(self._src_filename or 'memory'),
                    FUSE_REF_FILE=os.path.basename(self._ref_filename or 'memory'), FUSE_PROC_CRS=self._proc_crs.name,
                    **{f'FUSE_{k.upper()}': getattr(v, 'name', v) for k, v in settings.items()})
        if _is_path(corr_filename):
            levels, level_masks = overviews[0] if (mask is not None and overviews[0] is not None) else (overviews[0], None)
            self._save(corr_filename, corr, self._transform, nodata, meta, overviews=levels, compressor=compressor,
                       write_options=write_options, mask=mask, overview_masks=level_masks)
        if _is_path(param_filename):
            self._save(param_filename, params, self._param_grid.transform, float('nan'), meta, self._param_descriptions(n_param),
                       overviews=overviews[1], compressor=compressor, write_options=write_options)

    @staticmethod
    def _write_options(creation_options: Dict, tiff_dtypes: Sequence[Tuple[str, np.dtype]]) -> Dict:
        """ ``out_profile['creation_options']`` as the keyword arguments of ``tiff.write_tiff``: ``tile``, ``compress``,
        ``predictor``, ``bigtiff``.  Missing keys take the default profile's values (no predictor); a value of ``compress``,
        ``predictor``, ``blockxsize`` / ``blockysize``, ``bigtiff``, ``tiled`` or ``interleave`` that the writer cannot honour
        raises ``ValueError`` naming the key; every other key is ignored.  ``tiff_dtypes``: (name, sample dtype) of the files that are
        written as ``.tif``.  One profile shapes both files, as in the reference, so the predictor has to suit each of them: the
        parameter file is float32 whatever the output dtype, and an integer corrected file beside it leaves predictor 1 only. """
        from homonim_amd.tiff import bigtiff_wanted
        opts = dict(RasterFuse.create_out_profile()['creation_options'], predictor=1)
        opts.update({str(k).lower(): v for k, v in (creation_options or {}).items()})

        def refuse(key, what):
            raise ValueError(f"creation option `{key}`={opts[key]!r} cannot be written: {what}")

        compress = opts['compress']
        compress = None if compress is None or str(compress).lower() == 'none' else str(compress).lower()
        if compress not in (None, 'deflate'):
            refuse('compress', "'deflate' and None / 'none' are")
        try:
            predictor = int(opts['predictor'])
        except (TypeError, ValueError):
            predictor = 0
        if predictor not in (1, 2, 3):
            refuse('predictor', '1, 2 and 3 are')
        if predictor != 1 and compress is None:
            refuse('predictor', 'a predictor needs compress=deflate')
        for what, dt in tiff_dtypes:
            if (predictor == 2 and dt.kind == 'f') or (predictor == 3 and dt.kind != 'f'):
                refuse('predictor', f"2 is for integer samples and 3 for floats; {what} is '{dt.name}'")
        try:
            bx, by = int(opts['blockxsize']), int(opts['blockysize'])
        except (TypeError, ValueError):
            refuse('blockxsize', 'block sizes are integers')
        if bx != by:
            refuse('blockysize', f'tiles are square (blockxsize is {bx})')
        if bx < 16 or bx > 512 or bx % 16:
            refuse('blockxsize', 'a multiple of 16 in 16..512 is')
        try:
            bigtiff_wanted(opts['bigtiff'], 0, True, 0)
        except ValueError:
            refuse('bigtiff', "'yes', 'no', 'if_needed' and 'if_safer' are")
        if opts['tiled'] is not True and str(opts['tiled']).lower() not in ('true', 'yes', '1'):
            refuse('tiled', 'only tiled files are')
        if str(opts['interleave']).lower() != 'band':
            refuse('interleave', "only 'band' is")
        return dict(tile=bx, compress=compress is not None, predictor=predictor, bigtiff=opts['bigtiff'])

    @staticmethod
    def _pin(ctx, arrays) -> List[np.ndarray]:
        """ hipHostRegister the arrays that can be (C-contiguous, not page-locked yet); returns those that were. """
        done = []
        for arr in arrays:
            if arr is None or not isinstance(arr, np.ndarray) or not arr.flags['C_CONTIGUOUS'] or arr.nbytes == 0:
                continue
            try:
                ctx.pin(arr)   # counted per address range (Context.pin): concurrent process() calls share a registration
                done.append(arr)
            except DeviceError:
                pass  # not lockable (ulimit -l, foreign memory): the copies of this array stay synchronous
        return done

    @staticmethod
    def _run_blocks(blocks, fn, contexts, threads: int) -> List:
        """ ``fn(bp, worker_i)`` of every block, the results in block order.  Blocks are dealt round-robin to the workers, one per
        context; one thread with one context is a plain loop, anything else a pool of max(threads, contexts) threads.  A worker's
        exception is re-raised (fuse.py:404-408). """
        n = len(contexts)
        if threads == 1 and n == 1:
            return [fn(bp, 0) for bp in blocks]
        several = len({c.device for c in contexts}) > 1

        def on_device(bp, worker_i):
            # several GPUs in one process: the worker that packs this block into a GPU's pinned staging ring runs on that GPU's
            # NUMA node (topology.bind_current_thread; one process per GPU binds the whole process instead: dist / bench.py)
            if several:
                from homonim_amd import topology
                topology.bind_current_thread(contexts[worker_i].device)
            return fn(bp, worker_i)

        with ThreadPoolExecutor(max_workers=max(threads, n)) as ex:
            futures = [ex.submit(on_device, bp, i % n) for i, bp in enumerate(blocks)]
            return [f.result() for f in futures]

    def _param_descriptions(self, n_param: int) -> List[str]:
        """ Band descriptions of the parameter file (homonim/fuse.py:241-248): ``<ref band>_GAIN``, ``_OFFSET``, ``_R2`` in the
        file's band order, ``<ref band>`` being the reference band's own description or ``B<n>``. """
        n_src = self._src.shape[0]
        names = [(self._ref_descriptions[bi] if bi < len(self._ref_descriptions) else None) or f'B{bi + 1}' for bi in range(n_src)]
        return [f'{name}_{param}' for param in ('GAIN', 'OFFSET', 'R2')[:n_param] for name in names]

    @staticmethod
    def _is_tiff(filename) -> bool:
        return _is_path(filename) and os.fspath(filename).lower().endswith(('.tif', '.tiff'))

    @staticmethod
    def _overviews(ctx, array: np.ndarray, nodata, valid: Optional[np.ndarray] = None):
        """ The internal overviews of a finished (bands, H, W) raster (homonim/fuse.py:152-165), finest first; None when the
        raster is too small for one.  ``valid``: the raster's validity in place of a nodata value -- the masked build, which
        returns ``(levels, level_valids)``. """
        n_levels = len(overview_factors(array.shape[-2:]))
        return ctx.overviews(array, nodata, n_levels, valid=valid) if n_levels else None

    def _save(self, filename, array: np.ndarray, transform: Affine, nodata, metadata: Dict,
              descriptions: Optional[List[str]] = None, overviews: Optional[List[np.ndarray]] = None, compressor=None,
              write_options: Optional[Dict] = None, mask: Optional[np.ndarray] = None,
              overview_masks: Optional[List[np.ndarray]] = None):
        """ ``.tif`` / ``.tiff``: tiled GeoTIFF as ``write_options`` say (``_write_options``; None: the reference's default output
        profile), with ``overviews`` as its internal overviews when given, its tiles compressed by ``compressor``
        (``tiff.write_tiff``; None: host zlib), with ``mask`` / ``overview_masks`` as its internal masks; anything else:
        ``numpy.save`` (no mask). """
        if self._is_tiff(filename):
            from homonim_amd.tiff import write_tiff
            write_tiff(filename, array, transform, self._crs, nodata, {k: str(v) for k, v in metadata.items()},
                       descriptions=descriptions, overviews=overviews, mask=mask, overview_masks=overview_masks,
                       compressor=compressor if (write_options or {}).get('compress', True) else None, **(write_options or {}))
        else:
            np.save(filename, array)


def overview_factors(shape: Sequence[int], max_num_levels: int = 8, min_level_pixels: int = 256) -> List[int]:
    """ The decimation factors of the internal overviews of a raster of ``shape`` (rows, columns), as
    ``RasterFuse._build_overviews`` picks them (homonim/fuse.py:152-165): successive powers of 2 such that the coarsest level
    keeps at least ``min_level_pixels`` along the shorter dimension, ``max_num_levels`` at most; ``[]`` for a small raster. """
    height, width = int(shape[-2]), int(shape[-1])
    if height < 1 or width < 1:
        return []
    max_ovw_levels = min(height, width).bit_length() - 1   # int(min(log2(shape))), exactly
    n = min(int(max_num_levels), max_ovw_levels - int(math.log2(min_level_pixels)))
    return [2 ** m for m in range(1, n + 1)]


def convert_dtype(array: np.ndarray, dtype: str, nodata: Optional[float]) -> np.ndarray:
    """
    Host-side statement of ``RasterArray._convert_array_dtype`` (homonim/raster_array.py:353-387): round half-to-even and
    clip for integer types, NaN (the internal nodata) -> ``nodata``.  ``RasterFuse.process`` does this conversion on the
    device (hk_convert.hip); this helper documents the semantics and serves host-side callers.
    """
    has_nodata, nodata_value = _hk.out_nodata_code(dtype, nodata)   # refuses a nodata the dtype cannot hold (:357-358)
    invalid = np.isnan(array)
    out = array
    if np.issubdtype(np.dtype(dtype), np.integer):
        info = np.iinfo(dtype)
        out = np.clip(np.round(array.astype(np.promote_types(array.dtype, dtype))), info.min, info.max)
    with np.errstate(invalid='ignore', over='ignore'):
        out = out.astype(dtype, copy=(out is array))
    if has_nodata:
        out[invalid] = nodata_value
    elif np.issubdtype(np.dtype(dtype), np.integer):
        out[invalid] = 0   # the reference leaves NaN -> integer to the platform; the device's conversion gives 0 (hk_convert.hip)
    return out
