""" CPU tests of the parameter statistics' host side: GeoTIFF band descriptions (homonim_amd/tiff.py), validate_param_image
(homonim_amd/utils.py), and everything of ParamStats (homonim_amd/stats.py) that happens before or after the device reduction.
No GPU context is created here. """
import json
import os

import numpy as np
import pytest

from conftest import REPO
from homonim_amd import Affine, CRS, Model, ParamStats, utils
from homonim_amd import stats as stats_mod
from homonim_amd.errors import ImageFormatError, IoError
from homonim_amd.tiff import read_tiff, read_tiff_header, write_tiff

TIFF_DIR = os.path.join(REPO, 'tests', 'golden', 'tiff')
PARAM_FILES = [os.path.join(TIFF_DIR, n) for n in ('float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM.tif',
                                                   'float_100cm_rgb_FUSE_cREF_mGAIN-OFFSET_k5_5_PARAM_tile_10x20.tif')]
BYTE_FILE = os.path.join(REPO, 'tests', 'golden', 'rasters', 'ngi_rgb_byte_1.tif')
NAMES = ['B1_GAIN', 'B2_GAIN', 'B3_GAIN', 'B1_OFFSET', 'B2_OFFSET', 'B3_OFFSET', 'B1_R2', 'B2_R2', 'B3_R2']
TAGS = dict(FUSE_MODEL='gain_offset', FUSE_KERNEL_SHAPE='(5, 5)', FUSE_PROC_CRS='ref', FUSE_REF_FILE='ref.tif',
            FUSE_R2_INPAINT_THRESH='0.25')


# -- band descriptions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', PARAM_FILES)
def test_reference_param_files_carry_their_band_descriptions(path):
    tif = read_tiff(path)
    assert list(tif.descriptions) == NAMES
    header = read_tiff_header(path)
    assert list(header.descriptions) == NAMES
    assert (header.count, header.height, header.width, header.dtype) == (*tif.array.shape, 'float32')
    assert header.metadata == tif.metadata and header.metadata['FUSE_MODEL'] == 'gain_offset'
    assert 'DESCRIPTION' not in tif.metadata   # band items stay out of the dataset's
    assert header.transform == tif.transform and header.crs == tif.crs and np.isnan(header.nodata)


def test_descriptions_and_metadata_survive_a_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    array = rng.normal(size=(3, 21, 34)).astype(np.float32)
    meta = {'FUSE_MODEL': 'gain_offset', 'QUOTED': 'a "b" <c> & d'}
    names = ['red <1> & "x"', None, 'NIR_R2']
    path = tmp_path / 'd.tif'
    write_tiff(path, array, Affine(2., 0., 10., 0., -2., 50.), CRS('EPSG:32735'), float('nan'), meta, tile=16, descriptions=names)
    tif = read_tiff(path)
    assert tif.descriptions == tuple(names) and tif.metadata == meta
    assert np.array_equal(tif.array, array)
    assert read_tiff_header(path).descriptions == tuple(names)
    # descriptions alone, and none: files without them read as None per band
    write_tiff(tmp_path / 'e.tif', array, Affine.identity(), descriptions=['a', 'b', 'c'])
    assert read_tiff(tmp_path / 'e.tif').descriptions == ('a', 'b', 'c') and read_tiff(tmp_path / 'e.tif').metadata == {}
    write_tiff(tmp_path / 'f.tif', array, Affine.identity(), metadata=meta)
    assert read_tiff(tmp_path / 'f.tif').descriptions == (None, None, None)
    with pytest.raises(ValueError):
        write_tiff(tmp_path / 'g.tif', array, Affine.identity(), descriptions=['a'])


# -- validation --------------------------------------------------------------------------------------------------------------
def _write_param(path, count=9, names=None, tags=None):
    array = np.ones((count, 6, 7), np.float32)
    write_tiff(path, array, Affine.identity(), CRS(), float('nan'), TAGS if tags is None else tags,
               descriptions=NAMES[:count] if names is None else names)
    return path


def test_validate_param_image(tmp_path):
    for path in PARAM_FILES:
        assert utils.validate_param_image(path).count == 9
    assert utils.validate_param_image(_write_param(tmp_path / 'ok.tif')).descriptions == tuple(NAMES)
    lower = [n.lower() for n in NAMES]
    utils.validate_param_image(_write_param(tmp_path / 'lower.tif', names=lower))   # case-insensitive
    with pytest.raises(ImageFormatError):
        utils.validate_param_image(BYTE_FILE)
    with pytest.raises(ImageFormatError):   # gains and offsets swapped
        utils.validate_param_image(_write_param(tmp_path / 'names.tif', names=NAMES[3:6] + NAMES[:3] + NAMES[6:]))
    with pytest.raises(ImageFormatError):   # no descriptions at all
        utils.validate_param_image(_write_param(tmp_path / 'none.tif', names=[None] * 9))
    for missing in utils.PARAM_TAGS:
        tags = {k: v for k, v in TAGS.items() if k != missing}
        with pytest.raises(ImageFormatError):
            utils.validate_param_image(_write_param(tmp_path / f'{missing}.tif', tags=tags))
    with pytest.raises(ImageFormatError):   # 2 x bands: a fuse with find_r2 off
        utils.validate_param_image(_write_param(tmp_path / 'six.tif', count=8, names=NAMES[:8]))
    with pytest.raises(FileNotFoundError):
        utils.validate_param_image(tmp_path / 'missing.tif')
    with pytest.raises(FileNotFoundError):
        ParamStats(tmp_path / 'missing.tif')
    with pytest.raises(ImageFormatError):
        ParamStats(BYTE_FILE)


# -- the class, before any device call ---------------------------------------------------------------------------------------
def test_metadata_and_context_management():
    ps = ParamStats(PARAM_FILES[0])
    assert ps.closed
    meta = ps.metadata
    assert len(meta) > 0 and 'Model: gain-offset' in meta and 'Kernel shape: (5, 5)' in meta
    assert 'Processing CRS: ref' in meta and 'Reference: float_100cm_rgb.tif' in meta
    assert 'R\N{SUPERSCRIPT TWO} inpaint threshold: 0.25' in meta and len(meta.strip().split('\n')) == 5
    with pytest.raises(IoError):
        ps.stats()
    with pytest.raises(IoError):
        ps._get_data_window()
    with ps:
        assert not ps.closed
    assert ps.closed
    with pytest.raises(IoError):
        ps.stats()
    gain = ParamStats.from_arrays(np.ones((3, 4, 5), np.float32), Model.gain_blk_offset, kernel_shape=(3, 3), proc_crs='ref')
    assert not gain.closed and 'Model: gain-blk-offset' in gain.metadata and len(gain.metadata.strip().split('\n')) == 4
    gain.close()
    assert gain.closed
    with pytest.raises(IoError):
        gain.__enter__()
    with pytest.raises(ImageFormatError):
        ParamStats.from_arrays(np.ones((4, 4, 5), np.float32), Model.gain)


def _ref_image_stats(image_accum, names):
    """ homonim/stats.py:175-192 restated with numpy scalars """
    out = []
    for name, acc in zip(names, image_accum):
        n = np.float64(acc['n'])
        d = dict(band=name, mean=np.float64(acc['sum']) / n,
                 std=np.sqrt((np.float64(acc['sum2']) / n) - (np.float64(acc['sum']) ** 2 / n ** 2)), min=acc['min'], max=acc['max'])
        if 'inpaint_sum' in acc:
            d['inpaint_p'] = 100 * acc['inpaint_sum'] / n
        out.append(d)
    return out


def test_sums_to_statistics_follow_the_reference_formula():
    vectors = [
        [0.5, 2.5, 30.25, 101.5, 20, 3, 0, 0, 4, 3],
        [-3.0, 7.0, -11.0, 400.0, 12, 5, 1, 1, 3, 3],
        [0.0, 1.0, 9.75, 7.5, 13, 4, 0, 1, 4, 3],
        [1.0, 1.0, 20.0, 19.999999999999996, 20, 0, 0, 0, 4, 3],   # rounding makes the variance negative: NaN, unclamped
        [0.1, 0.9, 5.0, 3.0, 10, 2, 0, 0, 4, 3],
        [0.2, 0.8, 6.0, 4.0, 11, 6, 0, 0, 4, 3],
    ]
    names = ['B1_GAIN', 'B2_GAIN', 'B1_OFFSET', 'B2_OFFSET', 'B1_R2', 'B2_R2']
    ps = ParamStats.from_arrays(np.zeros((6, 4, 5), np.float32), Model.gain_offset, r2_inpaint_thresh=0.25)
    count = 6
    assert [ps._wants_inpaint(b, count) for b in range(count)] == [False] * 4 + [True] * 2   # band_i >= count * 2 / 3
    accum = [ps._band_accum(v, ps._wants_inpaint(b, count)) for b, v in enumerate(vectors)]
    assert accum[4] == dict(min=0.1, max=0.9, sum=5.0, sum2=3.0, n=10, inpaint_sum=2) and 'inpaint_sum' not in accum[0]
    with np.errstate(all='ignore'):
        expected = _ref_image_stats(accum, names)
    got = ps._get_image_stats(accum)
    for g, e in zip(got, expected):
        assert set(g) == set(e) | {'n'}
        for k, v in e.items():
            assert g[k] == v or (np.isnan(g[k]) and np.isnan(v)), (k, g, e)
    assert np.isnan(got[3]['std']) and got[4]['inpaint_p'] == 20.0 and got[5]['inpaint_p'] == 100 * 6 / 11
    assert [g['n'] for g in got] == [20, 12, 13, 20, 10, 11]
    # the empty band: NaN with n = 0 (the documented deviation)
    empty = ps._get_image_stats([ps._band_accum(stats_mod._empty_vector(4, 5), with_inpaint) for with_inpaint in (False, True)])
    for e in empty:
        assert e['n'] == 0 and all(np.isnan(e[k]) for k in ('mean', 'std', 'min', 'max'))
    assert np.isnan(empty[1]['inpaint_p']) and 'inpaint_p' not in empty[0]
    # other models and a missing threshold have no inpaint_p
    for other in (ParamStats.from_arrays(np.zeros((6, 4, 5), np.float32), Model.gain_blk_offset),
                  ParamStats.from_arrays(np.zeros((6, 4, 5), np.float32), Model.gain_offset, r2_inpaint_thresh=None)):
        assert not any(other._wants_inpaint(b, count) for b in range(count))


def test_strips_merge_exactly():
    """ min of mins, sum of sums, union of boxes with the strips' row offsets; an empty strip leaves the box alone """
    acc = stats_mod._empty_vector(30, 8)
    stats_mod._merge(acc, np.array([np.inf, -np.inf, 0, 0, 0, 0, 8, 10, -1, -1.]), 0)
    assert acc.tolist() == stats_mod._empty_vector(30, 8).tolist()
    stats_mod._merge(acc, np.array([1., 4., 10., 30., 5, 1, 2, 3, 6, 9.]), 10)
    stats_mod._merge(acc, np.array([-2., 3., 1., 9., 4, 2, 1, 0, 4, 5.]), 20)
    assert acc.tolist() == [-2., 4., 11., 39., 9, 3, 1, 13, 6, 25]
    stats_mod._merge(acc, np.array([np.nan, np.nan, np.nan, np.nan, 2, 0, 0, 0, 7, 0.]), 29)
    assert np.isnan(acc[:4]).all() and acc[4:].tolist() == [11, 3, 0, 13, 7, 29]
    ps = ParamStats.from_arrays(np.zeros((3, 10, 8), np.float32), Model.gain, strip_bytes=3 * 8 * 4)
    assert ps._strips([0, 2]) == [(0, 0, 3), (0, 3, 6), (0, 6, 9), (0, 9, 10), (2, 0, 3), (2, 3, 6), (2, 6, 9), (2, 9, 10)]
    assert ParamStats.from_arrays(np.zeros((3, 10, 8), np.float32), Model.gain, strip_bytes=1)._strips([1])[:2] == [(1, 0, 1), (1, 1, 2)]
    assert ParamStats.from_arrays(np.zeros((3, 10, 8), np.float32), Model.gain)._strips([1]) == [(1, 0, 10)]
    assert stats_mod.STRIP_BYTES == 64 << 20


def test_tables():
    stats_list = [dict(band='B1_GAIN', mean=1.23456, std=0.5, min=-0.25, max=2.0, n=7),
                  dict(band='B1_OFFSET', mean=-0.00001, std=0.125, min=-1.0, max=11.0625, n=7),
                  dict(band='B1_R2', mean=0.75, std=0.0625, min=0.0, max=1.0, inpaint_p=12.3456, n=7)]
    table = ParamStats.stats_table(stats_list)
    for band_stats in stats_list:
        for k, v in band_stats.items():
            if k != 'n':
                assert (f'{v:.3f}' in table) if isinstance(v, float) else (v in table)
    for schema_dict in ParamStats.schema.values():
        assert schema_dict['abbrev'] in table
    assert ''.join(table.split('\n')[0].split()) == 'BandMeanStd.Min.Max.Inpaint(%)'   # the reference's columns only
    assert ''.join(table.split('\n')[-1].split()) == 'B1_R20.7500.0620.0001.00012.346'
    assert ''.join(table.split('\n')[-2].split()) == 'B1_OFFSET-0.0000.125-1.00011.062'
    schema_table = ParamStats.schema_table()
    assert 'Inpaint (%)' in schema_table and '*_R2' in schema_table and 'ABBREV' in schema_table


# -- python -m homonim_amd.stats ---------------------------------------------------------------------------------------------
def test_command_line(tmp_path, monkeypatch, capsys):
    calls = []

    def fake_reduce(self, band_indexes, threads):
        calls.append((self._param_filename.name, list(band_indexes)))
        return [np.array([1., 1., 144., 144., 144, 0, 1, 1, 8, 18.]) for _ in band_indexes]

    monkeypatch.setattr(ParamStats, '_reduce', fake_reduce)
    out_file = tmp_path / 'stats.json'
    assert stats_mod.main([PARAM_FILES[0], PARAM_FILES[1], '--output', str(out_file)]) == 0
    printed = capsys.readouterr().out
    for path in PARAM_FILES:
        assert os.path.basename(path) in printed
    assert 'Model: gain-offset' in printed and 'Inpaint (%)' in printed and 'B3_R2' in printed
    assert [c[1] for c in calls] == [list(range(9))] * 2
    with open(out_file) as f:
        stats_dict = json.load(f)
    assert set(stats_dict) == set(PARAM_FILES)
    for stats_list in stats_dict.values():
        assert [s['band'] for s in stats_list] == NAMES
        assert all(s['mean'] == 1.0 and s['std'] == 0.0 and s['n'] == 144 for s in stats_list)
        assert all(('inpaint_p' in s) == (i >= 6) for i, s in enumerate(stats_list))
    # no --output: nothing is written; a file that is no parameter image or does not exist ends with a usage error
    assert stats_mod.main([PARAM_FILES[0]]) == 0
    for bad in (BYTE_FILE, str(tmp_path / 'missing.tif')):
        with pytest.raises(SystemExit) as ex:
            stats_mod.main([bad])
        assert ex.value.code != 0
        assert 'Invalid value' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        stats_mod.main([])


def test_raster_fuse_names_the_parameter_bands():
    """ fuse.py:241-248 of the reference: <reference band description or B<n>>_GAIN / _OFFSET / _R2 in the file's band order """
    from homonim_amd import RasterFuse
    fuse = RasterFuse(np.ones((2, 8, 8), np.float32), np.ones((2, 8, 8), np.float32))
    assert fuse._param_descriptions(3) == ['B1_GAIN', 'B2_GAIN', 'B1_OFFSET', 'B2_OFFSET', 'B1_R2', 'B2_R2']
    assert fuse._param_descriptions(2) == ['B1_GAIN', 'B2_GAIN', 'B1_OFFSET', 'B2_OFFSET']
    fuse._ref_descriptions = ('red', None)
    assert fuse._param_descriptions(3) == ['red_GAIN', 'B2_GAIN', 'red_OFFSET', 'B2_OFFSET', 'red_R2', 'B2_R2']
