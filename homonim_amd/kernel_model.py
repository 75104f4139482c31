"""
Sliding-window kernel models on the MI355X: host-side mirror of the reference's operator interface for the hot path.

Same class / method names, argument meaning and error behaviour as homonim/kernel_model.py (``KernelModel`` :35-463,
``RefSpaceModel`` :466-503, ``SrcSpaceModel`` :506-535), but ``fit`` / ``apply`` hand the block to hand-written HIP
kernels through the C ABI of include/homonim_hk.h (ctypes, ``homonim_amd/_hk.py``).  Nothing here computes pixels on
the CPU and there is no fallback: without the built library or a gfx950 device the calls raise ``DeviceError``.

Differences a caller can observe (all documented in DESIGN.md):

* ``fit`` does NOT zero-fill / normalise the caller's ``src_ra`` / ``ref_ra`` in place (the reference does,
  kernel_model.py:246-247,292-295,320-321; its own wrappers always pass temporaries or copies).
* ``fit_apply`` is an extra, fused entry point for ``RasterFuse._process_block``'s fit->apply pair (fuse.py:305-307).
  ``RefSpaceModel`` / ``SrcSpaceModel`` have it across grids as well: one call per block pair, typed blocks in, everything
  between them on the device (hk_refspace_fit_apply, hk_srcspace_fit_apply).
* gain-offset with ``r2_inpaint_thresh`` set: the kernel evaluates the r2 mask (kernel_model.py:363); when no valid
  pixel fails it the reference's GDAL ``fillnodata`` branch is the identity and results are identical; when some
  fail, the offsets are in-painted on the device by a restatement of GDAL's published fill algorithm (parity with
  GDAL itself unpinned, hk_inpaint.hip) and the gains of the failing pixels are recomputed as in :370-371.
* ``RefSpaceModel`` / ``SrcSpaceModel`` re-sample between same-CRS, axis-aligned grids on the device (every
  ``rasterio.enums.Resampling`` warp method: a restatement of GDAL's warp kernels, pinned against the real stack's
  published accuracy table for average / cubic_spline, otherwise unpinned); rasters of two CRSs (bring one to the other's
  with ``RasterArray.reproject(crs=...)``, as ``RasterFuse`` does) and rotations raise ``NotImplementedError``, ``gauss`` is
  rejected as in rasterio.
"""
from typing import Dict, Optional, Tuple

import numpy as np

from homonim_amd import _hk, utils
from homonim_amd.enums import Model, Resampling
from homonim_amd.raster_array import RasterArray


class KernelModel:
    default_kernel_shape = (5, 5)
    default_model = Model.gain_blk_offset

    def __init__(self, model: Model = default_model, kernel_shape: Tuple[int, int] = default_kernel_shape,
                 find_r2: bool = False, **kwargs):
        """
        model: correction model; kernel_shape: (height, width) of the sliding window, odd; find_r2: add an R2 band to
        the parameters; kwargs: see ``create_config`` (unknown keys raise TypeError, as in the reference).
        """
        self._model = Model(model)
        self._kernel_shape = utils.validate_kernel_shape(kernel_shape, model=self._model)
        self._find_r2 = find_r2
        config = self.create_config(**kwargs)
        self._r2_inpaint_thresh: Optional[float] = config['r2_inpaint_thresh']
        self._mask_partial: bool = config['mask_partial']
        self._downsampling: Resampling = config['downsampling']
        self._upsampling: Resampling = config['upsampling']
        self._ctx = None  # GPU context, created on first use

    # -- configuration (kernel_model.py:83-136) -----------------------------------------------------------------------
    @property
    def model(self) -> Model:
        return self._model

    @property
    def kernel_shape(self) -> Tuple[int, int]:
        return tuple(self._kernel_shape)

    @property
    def find_r2(self) -> bool:
        return self._find_r2

    @staticmethod
    def create_config(r2_inpaint_thresh: Optional[float] = 0.25, mask_partial: bool = False,
                      downsampling: Resampling = Resampling.average,
                      upsampling: Resampling = Resampling.cubic_spline) -> Dict:
        """ The model configuration dict accepted by ``__init__`` and ``RasterFuse.process`` (defaults = reference). """
        return dict(r2_inpaint_thresh=r2_inpaint_thresh, mask_partial=mask_partial, downsampling=downsampling,
                    upsampling=upsampling)

    def _get_resampling(self, from_res: Tuple[float, float], to_res: Tuple[float, float]):
        """ kernel_model.py:138-140 """
        return self._downsampling if np.prod(np.abs(from_res)) <= np.prod(np.abs(to_res)) else self._upsampling

    # -- device plumbing ----------------------------------------------------------------------------------------------
    @property
    def context(self) -> '_hk.Context':
        if self._ctx is None:
            self._ctx = _hk.default_context()
        return self._ctx

    @context.setter
    def context(self, ctx: '_hk.Context'):
        self._ctx = ctx

    @property
    def _emit_r2(self) -> bool:
        # kernel_model.py:252 (gain models) / :325 (gain-offset)
        return bool(self._find_r2 or (self._model == Model.gain_offset and self._r2_inpaint_thresh is not None))

    @property
    def n_param(self) -> int:
        """ The bands of the parameters: gain, offset and, when R2 is emitted, R2. """
        return 3 if self._emit_r2 else 2

    def _desc(self, src_ra: RasterArray, ref_ra: RasterArray):
        thresh = self._r2_inpaint_thresh if self._model == Model.gain_offset else None
        return _hk.make_desc(self._model, self._kernel_shape, self._find_r2, thresh, src_ra.nodata, ref_ra.nodata)

    @staticmethod
    def _band(ra: RasterArray, what: str) -> np.ndarray:
        arr = ra.array
        if arr.ndim == 3:
            if arr.shape[0] != 1:
                raise ValueError(f'`{what}` must hold a single band')
            arr = arr[0]
        return arr

    @staticmethod
    def _wrap(corr: np.ndarray, params: Optional[np.ndarray], src_ra: RasterArray, param_grid_ra: RasterArray,
              out_nodata: Optional[float], want_params: bool) -> Tuple[RasterArray, Optional[RasterArray]]:
        """ (corr_ra, param_ra | None) of the arrays a fused device call returned; count and dtype are the arrays' own.  The corrected
        block: one band of the output dtype with nodata ``out_nodata`` on the source block's grid.  The parameters: ``n_param`` float32
        bands with NaN nodata on ``param_grid_ra``'s grid -- the reference block for RefSpaceModel across grids, else the source block. """
        grid = param_grid_ra
        param_ra = RasterArray(params, grid.crs, grid.transform, nodata=RasterArray.default_nodata) if want_params else None
        return RasterArray(corr, src_ra.crs, src_ra.transform, nodata=out_nodata), param_ra

    # -- the hot path -------------------------------------------------------------------------------------------------
    def fit(self, src_ra: RasterArray, ref_ra: RasterArray) -> RasterArray:
        """
        Fit sliding kernel models to a source / reference block pair on the same grid (kernel_model.py:411-440).
        Returns the parameters: gains in band 0, offsets in band 1 and, when ``find_r2`` (or gain-offset with an
        ``r2_inpaint_thresh``), R2 in band 2; NaN where either input is nodata.
        """
        _require_shared_grid(ref_ra, src_ra, "'ref_ra' and 'src_ra'")
        params, _, _, n_fail = self.context.fit_apply(
            self._desc(src_ra, ref_ra), self._band(src_ra, 'src_ra'), self._band(ref_ra, 'ref_ra'), self.n_param,
            want_params=True, want_corr=False
        )
        return RasterArray(params, src_ra.crs, src_ra.transform, nodata=RasterArray.default_nodata)

    def apply(self, src_ra: RasterArray, param_ra: RasterArray) -> RasterArray:
        """ Corrected block = gain * source + offset (kernel_model.py:442-463). """
        _require_shared_grid(param_ra, src_ra, "'param_ra' and 'src_ra'")
        corr = self.context.apply(self._band(src_ra, 'src_ra'), param_ra.array)
        return RasterArray.from_profile(corr, param_ra.profile)

    def fit_apply(self, src_ra: RasterArray, ref_ra: RasterArray, want_params: bool = False,
                  out_dtype: str = RasterArray.default_dtype, out_nodata: Optional[float] = RasterArray.default_nodata,
                  want_valid: bool = False):
        """
        ``apply(src_ra, fit(src_ra.copy(), ref_ra))`` in ONE pass over the data (window sums, solve, R2 test and
        correction fused in a single kernel; each input byte is read once).  Returns (corr_ra, param_ra | None).

        ``out_dtype`` / ``out_nodata`` convert the corrected block on the device the way the reference converts it when
        writing (raster_array.py:353-387); integer ``src_ra`` / ``ref_ra`` arrays are converted to float32 on the device.
        ``want_valid``: returns (corr_ra, param_ra | None, valid) -- ``valid`` the block's uint8 validity, 255 where the float32
        corrected value is not NaN and 0 where it is: the ``mask`` of the reference's corrected ``RasterArray`` before its
        conversion, which an integer output without a nodata value cannot carry itself (raster_array.py:493-500).
        """
        _require_shared_grid(ref_ra, src_ra, "'ref_ra' and 'src_ra'")
        if want_valid:   # the block entry with the whole block as its window: the one that writes validity (hk_fit_apply_block_valid)
            h, w = src_ra.shape
            corr, valid = np.empty((h, w), np.dtype(out_dtype)), np.empty((h, w), np.uint8)
            params = np.empty((self.n_param, h, w), np.float32) if want_params else None
            self.context.fit_apply_block(self._desc(src_ra, ref_ra), self._band(src_ra, 'src_ra'), self._band(ref_ra, 'ref_ra'),
                                         (0, 0, h, w), corr, params, out_nodata=out_nodata, valid_dst=valid)
            return (*self._wrap(corr, params, src_ra, src_ra, out_nodata, want_params), valid)
        params, corr, _, n_fail = self.context.fit_apply(
            self._desc(src_ra, ref_ra), self._band(src_ra, 'src_ra'), self._band(ref_ra, 'ref_ra'), self.n_param,
            want_params=want_params, want_corr=True, out_dtype=out_dtype, out_nodata=out_nodata
        )
        return self._wrap(corr, params, src_ra, src_ra, out_nodata, want_params)

    def fuses_into(self, src_ra: RasterArray, ref_ra: RasterArray) -> bool:
        """ True when ``fit_apply_into`` covers this model configuration for the pair (base-class fit + apply on a shared
        grid, nothing between them): the wrappers narrow it. """
        return (ref_ra.transform == src_ra.transform) and (ref_ra.shape == src_ra.shape)

    def fit_apply_into(self, src_ra: RasterArray, ref_ra: RasterArray, window, corr_dst: np.ndarray,
                       params_dst: Optional[np.ndarray] = None, out_nodata: Optional[float] = RasterArray.default_nodata,
                       valid_dst: Optional[np.ndarray] = None) -> int:
        """
        ``fit_apply`` for the block loop of ``RasterFuse.process`` (homonim/fuse.py:295-319): the window
        ``(row0, col0, rows, cols)`` of the block -- its out-block, i.e. the block without the halo that
        raster_array.py:478-491 crops on writing -- goes straight into ``corr_dst`` / ``params_dst``, views of the
        caller's corrected / parameter rasters (their dtype is the output dtype).  One call = one upload of the read-block,
        one download of the out-block, one stream synchronisation; asynchronous when the rasters are page-locked.
        Returns the number of pixels that failed the r2 mask.  ``valid_dst``: a uint8 view of the caller's validity raster at the
        same window, filled with the out-block's validity (255 / 0, ``fit_apply``'s ``want_valid``).
        """
        _require_shared_grid(ref_ra, src_ra, "'ref_ra' and 'src_ra'")
        _, n_fail = self.context.fit_apply_block(
            self._desc(src_ra, ref_ra), self._band(src_ra, 'src_ra'), self._band(ref_ra, 'ref_ra'), window, corr_dst,
            params_dst, out_nodata=out_nodata, valid_dst=valid_dst
        )
        return n_fail

    def _two_grid_dev_job(self, src, ref, corr, params, valid, window, param_window, out_nodata, stream, scratch):
        """ What ``RefSpaceModel.fit_apply_dev`` / ``SrcSpaceModel.fit_apply_dev`` share: the refusals of ``fit_apply`` (two CRSs,
        rotated grids) in its words, and (desc, io, job) of the device call. """
        from types import SimpleNamespace
        a, b = (SimpleNamespace(crs=r.crs, transform=r.grid_transform, shape=r.shape[1:]) for r in (src, ref))
        _require_one_crs(a, b)
        if src.shape[0] != ref.shape[0] or corr.shape[0] != src.shape[0]:
            raise ValueError(f'`src`, `ref` and `corr` must hold the same number of bands, got {src.shape[0]}, {ref.shape[0]} and {corr.shape[0]}')
        if params is not None:
            if params.dtype != np.float32:
                raise ValueError('`params` must be float32')
            if params.shape[0] != self.n_param * src.shape[0]:
                raise ValueError(f'`params` must hold {self.n_param} planes per band ({self.n_param * src.shape[0]}), got {params.shape[0]}')
        if valid is not None and valid.dtype != np.uint8:
            raise ValueError('`valid` must be uint8')
        if corr.dtype.name not in _hk.DTYPE_CODES:
            raise ValueError(f'unsupported output dtype {corr.dtype}')
        desc = self._desc(src, ref)
        io = _hk.make_io_desc(src.dtype, ref.dtype, corr.dtype, out_nodata)
        scratch_ptr, scratch_bytes = scratch if scratch is not None else (0, 0)
        job = _hk.make_two_grid_job(src, ref, corr, params, valid, window, param_window, stream, scratch_ptr, scratch_bytes)
        return desc, io, job

    def block_norm(self, src_ra: RasterArray, ref_ra: RasterArray) -> np.ndarray:
        """ The [gain, offset] block normalisation of gain-blk-offset (kernel_model.py:216-229), float64[2]. """
        return self.context.block_norm(self._desc(src_ra, ref_ra), self._band(src_ra, 'src_ra'),
                                       self._band(ref_ra, 'ref_ra'))


def _require_shared_grid(a: RasterArray, b: RasterArray, names: str):
    """ The base-class fit / apply take one grid (kernel_model.py:411-463); ``names``: the two arguments as the message names them. """
    if (a.transform != b.transform) or (a.shape != b.shape):
        raise ValueError(f'{names} must have the same CRS, transform and shape')


def _same_grid(a: RasterArray, b: RasterArray) -> bool:
    return a.transform == b.transform and a.shape == b.shape and a.crs == b.crs


def _require_one_crs(a: RasterArray, b: RasterArray):
    """ The models work on one CRS (the reference's RasterPairReader hands them blocks it has brought to one, homonim/utils.py:190-209). """
    from homonim_amd.crs import same_crs
    if not same_crs(a.crs, b.crs):
        raise NotImplementedError(f'the kernel models take rasters of one CRS, got {a.crs!r} and {b.crs!r}: bring one to the '
                                  'other\'s with RasterArray.reproject(crs=...) first (RasterFuse does)')
    # ... and on axis-aligned grids: between two different grids the models re-sample with the footprint methods, which are not
    # built for rotated / sheared ones (RasterFuse brings such rasters north-up before it cuts blocks)
    from homonim_amd.geo import is_rotated
    if (is_rotated(a.transform) or is_rotated(b.transform)) and not _same_grid(a, b):
        raise NotImplementedError('re-projection between rotated / sheared grids is not built for the kernel models: bring the '
                                  'raster north-up with RasterArray.reproject first (RasterFuse does)')


def _dev_grid_mapping(to_raster, from_raster, host_form: str):
    """ ``geo.grid_mapping`` between the grids of two device rasters, `src` and `ref`.  A raster on the device is the caller's and is
    not flipped for it; ``host_form``: what ``fit_apply`` of the class does with host arrays whose grids run opposite ways. """
    from homonim_amd.geo import grid_mapping
    kx, ox, ky, oy = grid_mapping(to_raster.grid_transform, from_raster.grid_transform)
    if kx < 0 or ky < 0:
        raise ValueError(f"'src' and 'ref' have opposite orientations along an axis: a device raster is not flipped for the caller "
                         f'({host_form}); flip one of them on the device first')
    return kx, ox, ky, oy


def _same_dev_grid(a, b) -> bool:
    return a.grid_transform == b.grid_transform and a.shape[1:] == b.shape[1:] and a.crs == b.crs


_SHARED_GRID_DEV = ('`src` and `ref` share one grid: the device-resident form of that is hk_fit_apply_dev (Context.fit_apply_dev), '
                    'which already serves it')


def _full_coverage_mask(model: KernelModel, in_mask_ra: RasterArray, param_ra: RasterArray) -> np.ndarray:
    """
    kernel_model.py:375-409: the mask of parameter-grid pixels fully covered by the input mask (re-projected with
    `average`, >= 1), having parameters, and whose (kh+2) x (kw+2) neighbourhood is all of that kind (erosion with a zero
    border).  Returns a bool array on the parameter grid; evaluated on the device.
    """
    cover_ra = in_mask_ra.reproject(**param_ra.proj_profile, nodata=None, resampling=Resampling.average,
                                    context=model.context)
    _, _, mask = model.context.partial_mask(cover_ra.array, None, param_ra.array[:2], model.kernel_shape, want_mask=True,
                                            coverage=True)
    return mask.astype(bool)


class RefSpaceModel(KernelModel):
    """
    Parameters estimated on the reference grid (kernel_model.py:466-503): the source block is re-sampled to the
    reference grid for ``fit`` and the parameters are re-sampled back to the source grid for ``apply``.  Re-sampling
    runs on the GPU for same-CRS, axis-aligned grids (hk_resample.hip: a restatement of GDAL's warp kernels).
    """

    def fit(self, src_ra: RasterArray, ref_ra: RasterArray) -> RasterArray:
        _require_one_crs(src_ra, ref_ra)
        if not _same_grid(src_ra, ref_ra):  # identical grids: the reference's `average` re-sampling is the identity
            resampling = self._get_resampling(src_ra.res, ref_ra.res)
            src_ra = src_ra.reproject(**ref_ra.proj_profile, resampling=resampling, context=self.context)  # :480
        return KernelModel.fit(self, src_ra, ref_ra)

    def apply(self, src_ra: RasterArray, param_ra: RasterArray) -> RasterArray:
        _require_one_crs(src_ra, param_ra)
        if _same_grid(src_ra, param_ra):
            if self._mask_partial:
                # full-coverage mask of the source mask & parameters, eroded by (kh+2) x (kw+2), then apply (:493-503)
                _, corr, _ = self.context.partial_mask(
                    self._band(src_ra, 'src_ra'), src_ra.nodata, param_ra.array[:2], self._kernel_shape,
                    src=self._band(src_ra, 'src_ra'), want_corr=True
                )
                return RasterArray.from_profile(corr, param_ra.profile)
            # the reference keeps only gain & offset and re-masks them with the source mask (:487,:500); on a shared
            # grid the parameters are already nodata wherever the source is.
            return KernelModel.apply(self, src_ra, param_ra)

        _param_ra = RasterArray.from_profile(param_ra.array[:2], param_ra.profile)  # :487
        resampling = self._get_resampling(param_ra.res, src_ra.res)
        param_us_ra = _param_ra.reproject(**src_ra.proj_profile, resampling=resampling, context=self.context)  # :491
        if self._mask_partial:
            mask = _full_coverage_mask(self, src_ra.mask_ra, _param_ra)  # :495
            mask_ra = RasterArray(mask.astype('float32'), _param_ra.crs, _param_ra.transform, nodata=None)
            mask_us_ra = mask_ra.reproject(**src_ra.proj_profile, nodata=0, resampling=Resampling.nearest,
                                           context=self.context)  # :497
            param_us_ra.mask = mask_us_ra.array.astype('bool', copy=False)  # :498
        else:
            param_us_ra.mask = src_ra.mask  # :500
        return KernelModel.apply(self, src_ra, param_us_ra)


    def fuses_into(self, src_ra: RasterArray, ref_ra: RasterArray) -> bool:
        return _same_grid(src_ra, ref_ra) and not self._mask_partial

    def fit_apply(self, src_ra: RasterArray, ref_ra: RasterArray, want_params: bool = False,
                  out_dtype: str = RasterArray.default_dtype, out_nodata: Optional[float] = RasterArray.default_nodata,
                  want_valid: bool = False):
        """ ``apply(src_ra, fit(src_ra, ref_ra))`` with everything between the two blocks kept in HBM
        (hk_refspace_fit_apply): one upload of source + reference, one download of the corrected block.  ``want_valid``: as in
        ``KernelModel.fit_apply`` (here the validity carries ``mask_partial``'s erosion as well). """
        if _same_grid(src_ra, ref_ra) and not self._mask_partial:
            return KernelModel.fit_apply(self, src_ra, ref_ra, want_params, out_dtype, out_nodata, want_valid)
        from homonim_amd.geo import grid_mapping
        _require_one_crs(src_ra, ref_ra)
        down = self._get_resampling(src_ra.res, ref_ra.res)
        up = self._get_resampling(ref_ra.res, src_ra.res)
        params, corr, _, *valid = self.context.refspace_fit_apply(
            self._desc(src_ra, ref_ra), self._band(src_ra, 'src_ra'), self._band(ref_ra, 'ref_ra'),
            grid_mapping(src_ra.transform, ref_ra.transform), grid_mapping(ref_ra.transform, src_ra.transform), int(down),
            int(up), self._mask_partial, self.n_param, want_params, out_dtype=out_dtype, out_nodata=out_nodata,
            want_valid=want_valid
        )
        return (*self._wrap(corr, params, src_ra, ref_ra, out_nodata, want_params), *valid)


    def fit_apply_dev(self, src, ref, corr, params=None, valid=None, window=None, param_window=None,
                      out_nodata: Optional[float] = RasterArray.default_nodata, stream: int = 0, scratch=None) -> np.ndarray:
        """ ``fit_apply`` of every band of two rasters that are resident on the device (hk_refspace_fit_apply_dev): nothing is
        staged, the call queues its work on pooled stream ``stream`` and returns the per-band r2-mask failure counts.
        ``src`` / ``ref``: ``_hk.DeviceRaster`` blocks with their transform, CRS and nodata; ``corr`` (the output dtype is its
        dtype), ``valid`` (uint8) and ``params`` (float32, ``n_param`` x bands planes, parameter-major, on the REFERENCE grid):
        device rasters whose ``dptr`` is the place of the window's first pixel.  ``window`` / ``param_window``: (row0, col0, rows,
        cols) of the source block / the reference block that is stored, None for the whole.  ``scratch``: (dptr, bytes) of
        ``Context.refspace_dev_scratch_bytes`` bytes, or None for the stream's own.  The bytes are ``fit_apply``'s, band by band. """
        if _same_dev_grid(src, ref) and not self._mask_partial:
            raise ValueError(_SHARED_GRID_DEV)
        desc, io, job = self._two_grid_dev_job(src, ref, corr, params, valid, window, param_window, out_nodata, stream, scratch)
        down = self._get_resampling(src.res, ref.res)
        up = self._get_resampling(ref.res, src.res)
        down_map, up_map = (_dev_grid_mapping(a, b, 'fit_apply passes such host arrays on and the library refuses their mapping')
                            for a, b in ((src, ref), (ref, src)))
        return self.context.refspace_fit_apply_dev(desc, down_map, up_map, int(down), int(up), self._mask_partial, job, io)

    def dev_scratch_bytes(self, src, ref, corr, params=None, valid=None, window=None, param_window=None,
                          out_nodata: Optional[float] = RasterArray.default_nodata) -> int:
        """ The bytes of ``scratch`` that ``fit_apply_dev`` of the same arguments needs (hk_refspace_dev_scratch_bytes: host arithmetic,
        no device; the pointers are looked at for NULL only), 0 for arguments the entry would refuse. """
        desc, io, job = self._two_grid_dev_job(src, ref, corr, params, valid, window, param_window, out_nodata, 0, None)
        down_map, up_map = (_dev_grid_mapping(a, b, 'fit_apply passes such host arrays on and the library refuses their mapping')
                            for a, b in ((src, ref), (ref, src)))
        return _hk.refspace_dev_scratch_bytes(desc, _hk.make_space_desc(down_map, up_map, int(self._get_resampling(src.res, ref.res)),
                                                                        int(self._get_resampling(ref.res, src.res)), self._mask_partial),
                                              job, io)


class SrcSpaceModel(KernelModel):
    """ Parameters estimated on the source grid (kernel_model.py:506-535): the reference block is re-sampled to it. """

    def fit(self, src_ra: RasterArray, ref_ra: RasterArray) -> RasterArray:
        _require_one_crs(src_ra, ref_ra)
        ref_us_ra = ref_ra
        if not _same_grid(src_ra, ref_ra):
            resampling = self._get_resampling(ref_ra.res, src_ra.res)
            ref_us_ra = ref_ra.reproject(**src_ra.proj_profile, resampling=resampling, context=self.context)  # :520
        param_ra = KernelModel.fit(self, src_ra, ref_us_ra)
        if self._mask_partial:
            # full-coverage mask of the reference mask & gain/offset, eroded by (kh+2) x (kw+2), on all bands (:526-531)
            if _same_grid(src_ra, ref_ra):
                masked, _, _ = self.context.partial_mask(
                    self._band(ref_ra, 'ref_ra'), ref_ra.nodata, param_ra.array, self._kernel_shape, want_params=True
                )
                param_ra = RasterArray.from_profile(masked, param_ra.profile)
            else:
                param_ra.mask = _full_coverage_mask(self, ref_ra.mask_ra, param_ra)
        elif not _same_grid(src_ra, ref_ra):
            param_ra.mask = src_ra.mask  # :533 (a no-op on a shared grid)
        return param_ra

    def fuses_into(self, src_ra: RasterArray, ref_ra: RasterArray) -> bool:
        return _same_grid(src_ra, ref_ra) and not self._mask_partial

    def fit_apply(self, src_ra: RasterArray, ref_ra: RasterArray, want_params: bool = False,
                  out_dtype: str = RasterArray.default_dtype, out_nodata: Optional[float] = RasterArray.default_nodata,
                  want_valid: bool = False):
        """ One fused pass on a shared grid.  Across grids everything between the two blocks stays in HBM as well
        (hk_srcspace_fit_apply): one upload of source + reference in their own dtypes, one download of the corrected block; with
        `average` the reference block -- the finer, larger one -- is read once, by the kernel that forms the averaged value and
        the coverage fraction of ``mask_partial`` together.  ``mask_partial`` on a shared grid keeps the reference's own sequence
        ``apply(src_ra, fit(src_ra, ref_ra))`` -- SrcSpaceModel.fit masks the parameters with the eroded full-coverage mask
        (kernel_model.py:526-531), which the fused kernel does not know about.  ``want_valid``: as in ``KernelModel.fit_apply``; that
        sequence has its float32 corrected block on the host, and its validity is read from it there. """
        if self.fuses_into(src_ra, ref_ra):
            return KernelModel.fit_apply(self, src_ra, ref_ra, want_params, out_dtype, out_nodata, want_valid)
        _require_one_crs(src_ra, ref_ra)
        if not _same_grid(src_ra, ref_ra):
            from homonim_amd.geo import grid_mapping
            kx, ox, ky, oy = grid_mapping(ref_ra.transform, src_ra.transform)
            ref = self._band(ref_ra, 'ref_ra')
            # grids of opposite orientation along an axis: flip the reference along it, as RasterArray.reproject does
            if ky < 0:
                ref, ky, oy = ref[::-1, :], -ky, ref.shape[0] - oy
            if kx < 0:
                ref, kx, ox = ref[:, ::-1], -kx, ref.shape[1] - ox
            params, corr, _, *valid = self.context.srcspace_fit_apply(
                self._desc(src_ra, ref_ra), self._band(src_ra, 'src_ra'), ref, (kx, ox, ky, oy),
                int(self._get_resampling(ref_ra.res, src_ra.res)), self._mask_partial, self.n_param, want_params,
                out_dtype=out_dtype, out_nodata=out_nodata, want_valid=want_valid
            )
            return (*self._wrap(corr, params, src_ra, src_ra, out_nodata, want_params), *valid)
        param_ra = self.fit(src_ra.copy(), ref_ra)
        corr_ra = self.apply(src_ra, param_ra)
        valid = (~np.isnan(corr_ra.array)).astype(np.uint8) * np.uint8(255) if want_valid else None
        if np.dtype(out_dtype) != np.float32 or not (out_nodata is None or (isinstance(out_nodata, float) and np.isnan(out_nodata))):
            from homonim_amd.fuse import convert_dtype
            arr = convert_dtype(corr_ra.array, str(np.dtype(out_dtype)), out_nodata)
            corr_ra = RasterArray.from_profile(arr, dict(corr_ra.profile, nodata=out_nodata, dtype=str(np.dtype(out_dtype))))
        if want_valid:
            return corr_ra, (param_ra if want_params else None), (valid[0] if valid.ndim == 3 else valid)
        return corr_ra, (param_ra if want_params else None)

    def fit_apply_dev(self, src, ref, corr, params=None, valid=None, window=None, param_window=None,
                      out_nodata: Optional[float] = RasterArray.default_nodata, stream: int = 0, scratch=None) -> np.ndarray:
        """ ``RefSpaceModel.fit_apply_dev`` for this model (hk_srcspace_fit_apply_dev): the parameters, and ``param_window``, are on
        the SOURCE grid.  A shared grid is refused: without ``mask_partial`` hk_fit_apply_dev serves it, with it ``fit_apply`` runs a
        host sequence that has no device-resident form. """
        if _same_dev_grid(src, ref):
            raise ValueError(_SHARED_GRID_DEV if not self._mask_partial else
                             '`src` and `ref` share one grid: SrcSpaceModel with mask_partial has no device-resident form there')
        desc, io, job = self._two_grid_dev_job(src, ref, corr, params, valid, window, param_window, out_nodata, stream, scratch)
        mapping = _dev_grid_mapping(ref, src, 'fit_apply flips the host array')
        return self.context.srcspace_fit_apply_dev(desc, mapping, int(self._get_resampling(ref.res, src.res)), self._mask_partial, job, io)

    def dev_scratch_bytes(self, src, ref, corr, params=None, valid=None, window=None, param_window=None,
                          out_nodata: Optional[float] = RasterArray.default_nodata) -> int:
        """ ``RefSpaceModel.dev_scratch_bytes`` for this model (hk_srcspace_dev_scratch_bytes) """
        desc, io, job = self._two_grid_dev_job(src, ref, corr, params, valid, window, param_window, out_nodata, 0, None)
        mapping = _dev_grid_mapping(ref, src, 'fit_apply flips the host array')
        return _hk.srcspace_dev_scratch_bytes(desc, _hk.make_srcspace_desc(mapping, int(self._get_resampling(ref.res, src.res)),
                                                                           self._mask_partial), job, io)
