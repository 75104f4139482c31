"""
``ParamStats``: the statistics the reference reports for a parameter image (homonim/stats.py, the ``homonim stats``
command) -- per parameter band the mean, standard deviation, minimum and maximum of the valid pixels and, for the R2 bands
of a gain-offset image, the portion of pixels that were in-painted.

Same surface as the reference class: ``ParamStats(param_filename)`` validates the file on construction
(``utils.validate_param_image``, header only), ``with`` opens it, ``metadata``, ``schema``, ``schema_table``,
``stats(threads) -> [ {band, mean, std, min, max[, inpaint_p]}, ... ]``, ``stats_table``, ``_get_data_window``.
``ParamStats.from_arrays`` takes the ``params`` array ``RasterFuse.process`` returns instead of a file.

The per-band reduction -- masked min, max, sum x, sum x^2, N, N(x < threshold) and the bounding box of the valid pixels --
runs on the GPU (``hk_param_stats``: one read of the band, float64 accumulation).  A band is handed over in strips of whole
rows of at most ``STRIP_BYTES`` (64 MiB: eight chunks of the context's 8 MiB pinned staging ring), so the device slab of a
stream slot stays bounded whatever the raster's size; strips are spread over the context's streams by ``threads`` and
accumulated in strip order (min of mins, sum of sums, union of boxes), so the result does not depend on ``threads``.

Deviations from the reference:
  * a band without a valid pixel gives NaN for mean / std / min / max with ``n`` = 0 (the reference divides by zero and passes
    numpy's ``masked`` along);
  * a file without a FUSE_R2_INPAINT_THRESH tag, or with ``None`` there (``from_arrays(..., r2_inpaint_thresh=None)``), has
    no ``inpaint_p``;
  * the sums are float64 sums of the float64 terms in a fixed GPU order; numpy's pairwise order differs in the last bits;
  * every dict also carries ``n``, the number of valid pixels (not tabulated: ``stats_table`` prints the reference's columns).

    python -m homonim_amd.stats FILE [FILE ...] [--output stats.json]
"""
import argparse
import json
import os
import pathlib
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from homonim_amd import _hk, utils
from homonim_amd.enums import Model
from homonim_amd.errors import ImageFormatError, IoError
from homonim_amd.geo import Window

# most bytes of a band handed to the device in one call (whole rows; at least one row)
STRIP_BYTES = 64 << 20

_MIN, _MAX, _SUM, _SUM2, _N, _N_BELOW, _COL_MIN, _ROW_MIN, _COL_MAX, _ROW_MAX = range(_hk.PARAM_STATS_N)


def _parse_thresh(text) -> Optional[float]:
    """ The FUSE_R2_INPAINT_THRESH tag (the reference reads it with yaml.safe_load): a number, or None / null. """
    if text is None or str(text).strip().lower() in ('', 'none', 'null', '~'):
        return None
    return float(text)


def _empty_vector(height: int, width: int) -> np.ndarray:
    return np.array([np.inf, -np.inf, 0., 0., 0., 0., width, height, -1., -1.])


def _merge(acc: np.ndarray, strip: np.ndarray, row_off: int):
    """ Fold the vector of a strip of rows starting at ``row_off`` into the band's (in place). """
    acc[_MIN], acc[_MAX] = np.minimum(acc[_MIN], strip[_MIN]), np.maximum(acc[_MAX], strip[_MAX])   # (NaN propagates)
    acc[_SUM:_N_BELOW + 1] += strip[_SUM:_N_BELOW + 1]
    if strip[_N] > 0:
        acc[_COL_MIN], acc[_COL_MAX] = min(acc[_COL_MIN], strip[_COL_MIN]), max(acc[_COL_MAX], strip[_COL_MAX])
        acc[_ROW_MIN], acc[_ROW_MAX] = min(acc[_ROW_MIN], strip[_ROW_MIN] + row_off), max(acc[_ROW_MAX], strip[_ROW_MAX] + row_off)


class ParamStats:
    """ Statistics of a parameter image, as created by ``RasterFuse.process(param_filename=...)``. """

    schema = dict(
        band=dict(abbrev='Band'),
        mean=dict(abbrev='Mean'),
        std=dict(abbrev='Std.'),
        min=dict(abbrev='Min.'),
        max=dict(abbrev='Max.'),
        inpaint_p=dict(abbrev='Inpaint (%)', description='Portion of inpainted pixels (%).'),
    )  # yapf: disable

    def __init__(self, param_filename: Union[str, os.PathLike], context: Optional['_hk.Context'] = None,
                 strip_bytes: Optional[int] = None, inflate: str = 'host'):
        """ ``context``: the GPU context to reduce on (default: the process-wide one, created on first use).
        ``strip_bytes``: see ``STRIP_BYTES``.  ``inflate``: who inflates the file's DEFLATE blocks: 'host' (default) -- zlib on
        the reading thread; 'device' -- ``Context.inflate_image`` of the same context: the same pixels.  The LZW blocks of a file
        go to the library's host decoder (``_hk.lzw_image_host``) under 'host' and to ``Context.lzw_image`` under 'device'. """
        _hk.block_decoders(inflate)   # (refuses anything but 'host' and 'device')
        self._inflate = inflate
        self._param_filename = pathlib.Path(param_filename)
        header = utils.validate_param_image(self._param_filename)
        self._init(header.metadata, header.descriptions, context, strip_bytes)
        self._from_file = True
        self._array = None   # read on __enter__

    def _init(self, tags: Dict[str, str], band_names: Sequence[str], context, strip_bytes):
        self._tags = dict(tags)
        self._band_names = list(band_names)
        self._model = str(self._tags['FUSE_MODEL']).replace('_', '-')
        self._r2_inpaint_thresh = _parse_thresh(self._tags.get('FUSE_R2_INPAINT_THRESH'))
        self._context = context
        self._strip_bytes = int(strip_bytes) if strip_bytes else None

    @classmethod
    def from_arrays(cls, params: np.ndarray, model: Union[Model, str], r2_inpaint_thresh: Optional[float] = 0.25,
                    band_names: Optional[Sequence[str]] = None, kernel_shape=None, proc_crs=None, ref_file: str = 'memory',
                    context: Optional['_hk.Context'] = None, strip_bytes: Optional[int] = None) -> 'ParamStats':
        """ Statistics of an in-memory parameter raster, e.g. the ``params`` ``RasterFuse.process`` returns: (3 x bands, height,
        width), gains first, then offsets, then R2, NaN where there is no data.  The object is open until ``close()`` / the end
        of a ``with`` block.  ``model`` and ``r2_inpaint_thresh`` are those of the fuse; ``band_names`` default to
        ``B<n>_GAIN``, ``B<n>_OFFSET``, ``B<n>_R2``. """
        params = np.asarray(params)
        if params.ndim != 3 or params.shape[0] == 0 or params.shape[0] % 3 != 0 or params.shape[1] == 0 or params.shape[2] == 0:
            raise ImageFormatError('`params` is not a parameter raster: (3 x bands, height, width) is expected.')
        n_refl = params.shape[0] // 3
        if band_names is None:
            band_names = [f'B{bi + 1}_{name}' for name in ('GAIN', 'OFFSET', 'R2') for bi in range(n_refl)]
        if len(band_names) != params.shape[0]:
            raise ValueError(f'{len(band_names)} band names for {params.shape[0]} bands')
        self = cls.__new__(cls)
        self._param_filename = pathlib.Path('memory')
        tags = dict(FUSE_MODEL=Model(getattr(model, 'value', model)).name, FUSE_KERNEL_SHAPE=str(kernel_shape),
                    FUSE_PROC_CRS=str(getattr(proc_crs, 'name', proc_crs)), FUSE_REF_FILE=str(ref_file),
                    FUSE_R2_INPAINT_THRESH=str(r2_inpaint_thresh))
        self._init(tags, band_names, context, strip_bytes)
        self._from_file = False
        self._array = params if params.dtype == np.float32 else params.astype(np.float32)
        return self

    # -- the reference's surface ----------------------------------------------------------------------------------------
    @property
    def closed(self) -> bool:
        """ True if the parameter file is closed, otherwise False. """
        return self._array is None

    @property
    def metadata(self) -> str:
        """ Parameter metadata string (stats.py:81-91). """
        res_str = (
            f'Model: {self._model}\n'
            f'Kernel shape: {self._tags["FUSE_KERNEL_SHAPE"]}\n'
            f'Processing CRS: {self._tags["FUSE_PROC_CRS"]}\n'
            f'Reference: {self._tags["FUSE_REF_FILE"]}\n'
        )
        if self._model == 'gain-offset':
            res_str += f'R\N{SUPERSCRIPT TWO} inpaint threshold: {self._r2_inpaint_thresh}\n'
        return res_str

    @staticmethod
    def schema_table() -> str:
        """ A table string describing the statistics returned by ``stats`` (stats.py:94-99). """
        from tabulate import tabulate
        schema_list = [v for k, v in ParamStats.schema.items() if 'description' in v]
        schema_list.append(dict(abbrev='*_R2', description='R\N{SUPERSCRIPT TWO} coefficient of determination.'))
        headers = {k: k.upper() for k in schema_list[0].keys()}
        return tabulate(schema_list, headers=headers, tablefmt='simple')

    @staticmethod
    def stats_table(stats_list: List[Dict]) -> str:
        """ A table string of the statistics ``stats`` returned (stats.py:102-117): the schema's columns. """
        from tabulate import tabulate
        headers = {k: v['abbrev'] for k, v in ParamStats.schema.items() if k in stats_list[-1]}
        rows = [{k: v for k, v in band_stats.items() if k in ParamStats.schema} for band_stats in stats_list]
        return tabulate(rows, headers=headers, floatfmt='.3f', stralign='right', tablefmt='simple')

    def __enter__(self):
        if self._array is None:
            if not self._from_file:
                raise IoError('The parameter raster has been closed')
            from homonim_amd.tiff import read_tiff
            inflater, lzw = _hk.block_decoders(getattr(self, '_inflate', 'host'), self._get_context)
            array = read_tiff(self._param_filename, inflater=inflater, lzw=lzw).array
            self._array = np.ascontiguousarray(array, dtype=np.float32)
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        self.close()

    def close(self):
        self._array = None

    def _assert_open(self):
        if self.closed:
            raise IoError(f'The parameter file has not been opened: {self._param_filename.name}')

    def _wants_inpaint(self, band_i: int, count: int) -> bool:
        """ stats.py:226: the R2 bands of a gain-offset image (and a threshold to compare with) """
        return self._model == Model.gain_offset.value and band_i >= count * 2 / 3 and self._r2_inpaint_thresh is not None

    @staticmethod
    def _band_accum(vector: Sequence[float], with_inpaint: bool) -> Dict:
        """ The reference's block dictionary (stats.py:223-229) from the device's vector of a band """
        accum = dict(min=float(vector[_MIN]), max=float(vector[_MAX]), sum=float(vector[_SUM]), sum2=float(vector[_SUM2]),
                     n=int(vector[_N]))
        if with_inpaint:
            accum.update(inpaint_sum=int(vector[_N_BELOW]))
        return accum

    def _get_image_stats(self, image_accum: List[Dict]) -> List[Dict]:
        """ Image statistics from accumulated results (stats.py:175-192; the formulas verbatim). """
        image_stats = []
        for band_i, band_accum in enumerate(image_accum):
            n = int(band_accum['n'])
            if n == 0:
                band_stats = dict(band=self._band_names[band_i], mean=float('nan'), std=float('nan'), min=float('nan'),
                                  max=float('nan'))
                if 'inpaint_sum' in band_accum:
                    band_stats['inpaint_p'] = float('nan')
            else:
                with np.errstate(all='ignore'):
                    s, s2, nf = np.float64(band_accum['sum']), np.float64(band_accum['sum2']), np.float64(n)
                    band_stats = dict(
                        band=self._band_names[band_i],
                        mean=float(s / nf),
                        # formula for cumulative std dev from https://rosettacode.org/wiki/Cumulative_standard_deviation#Python
                        std=float(np.sqrt((s2 / nf) - (s ** 2 / nf ** 2))),
                        min=float(band_accum['min']),
                        max=float(band_accum['max']),
                    )
                if 'inpaint_sum' in band_accum:
                    band_stats['inpaint_p'] = float(100 * band_accum['inpaint_sum'] / n)
            band_stats['n'] = n
            image_stats.append(band_stats)
        return image_stats

    # -- the reduction ---------------------------------------------------------------------------------------------------
    def _get_context(self) -> '_hk.Context':
        if self._context is None:
            dev = int(os.environ.get('HOMONIM_AMD_DEVICE', os.environ.get('LOCAL_RANK', '0')))
            self._context = _hk.get_context(dev)
        return self._context

    def _strips(self, band_indexes: Sequence[int]):
        """ (band, first row, end row) of every call: whole rows, at most the strip bound each """
        _, height, width = self._array.shape
        rows = max(1, (self._strip_bytes or STRIP_BYTES) // (4 * width))
        return [(bi, r0, min(r0 + rows, height)) for bi in band_indexes for r0 in range(0, height, rows)]

    def _reduce(self, band_indexes: Sequence[int], threads: int) -> List[np.ndarray]:
        """ The device's vector [min, max, sum, sum2, N, N_below, col_min, row_min, col_max, row_max] of each band asked for """
        count, height, width = self._array.shape
        ctx = self._get_context()
        strips = self._strips(band_indexes)

        def strip_vector(strip):
            bi, r0, r1 = strip
            thresh = self._r2_inpaint_thresh if self._wants_inpaint(bi, count) else None
            return ctx.param_stats(self._array[bi, r0:r1], float('nan'), thresh)

        workers = max(1, min(threads, ctx.n_streams, len(strips)))  # a thread beyond the streams would only wait for a slot
        if workers == 1:
            vectors = [strip_vector(s) for s in strips]
        else:
            with ThreadPoolExecutor(max_workers=workers) as ex:
                vectors = list(ex.map(strip_vector, strips))   # strip order: the accumulation does not depend on `threads`
        accs = {bi: _empty_vector(height, width) for bi in band_indexes}
        for (bi, r0, _), vec in zip(strips, vectors):
            _merge(accs[bi], vec, r0)
        return [accs[bi] for bi in band_indexes]

    def _get_data_window(self, threads: int = 0) -> Optional[Window]:
        """ The window of band 1's valid pixels (stats.py:135-173), or None when it has none. """
        self._assert_open()
        vec = self._reduce([0], utils.validate_threads(threads))[0]
        if vec[_N] == 0:
            return None
        return Window(int(vec[_COL_MIN]), int(vec[_ROW_MIN]), int(vec[_COL_MAX] - vec[_COL_MIN]) + 1,
                      int(vec[_ROW_MAX] - vec[_ROW_MIN]) + 1)

    def stats(self, threads: int = 0) -> List[Dict]:
        """ Parameter image statistics: one dictionary per band (stats.py:194-262).  ``threads``: strips in flight at a time
        (0 = as many as the context has streams). """
        self._assert_open()
        threads = utils.validate_threads(threads)
        count = self._array.shape[0]
        vectors = self._reduce(list(range(count)), threads)
        return self._get_image_stats([self._band_accum(vec, self._wants_inpaint(bi, count)) for bi, vec in enumerate(vectors)])


def main(argv: Optional[Sequence[str]] = None) -> int:
    """ ``python -m homonim_amd.stats``: report parameter statistics, as ``homonim stats`` does (cli.py). """
    parser = argparse.ArgumentParser(prog='python -m homonim_amd.stats', description='Report parameter statistics.')
    parser.add_argument('param_files', nargs='+', metavar='FILE', help='Path(s) to parameter image(s).')
    parser.add_argument('-o', '--output', metavar='FILE', default=None, help='Write results to this json file.')
    parser.add_argument('--inflate', choices=('host', 'device'), default='host',
                        help="Who decodes the files' DEFLATE and LZW blocks: the host (default) or the GPU.")
    args = parser.parse_args(argv)
    param_stats = []
    for name in args.param_files:
        try:
            param_stats.append(ParamStats(name, inflate=args.inflate))
        except (FileNotFoundError, ImageFormatError) as ex:
            parser.error(f"Invalid value for 'FILE': {ex}")
    stats_dict = {}
    for ps in param_stats:
        with ps:
            stats_dict[str(ps._param_filename)] = ps.stats()
        print(f'\n\n{ps._param_filename.name}:\n\n{ps.metadata}\nStats:\n\n{ps.stats_table(stats_dict[str(ps._param_filename)])}')
    if args.output:
        with open(args.output, 'w') as f:
            json.dump(stats_dict, f, indent=4)
    return 0


if __name__ == '__main__':
    sys.exit(main())
