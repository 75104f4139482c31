""" The resident mode of RasterFuse.process (device_config resident=True) as far as it goes without a GPU: the switch and the refusals
that need no library call, the grouping of a block list into device calls, and the two entries it adds (hk_fill_planes_dev,
hk_boundless_window_dev): symbols, argument types, rows in INTEGRATION.md, and the refusal of a NULL context. """
import ctypes
import os
import re

import numpy as np
import pytest

import _process_blocks as pb
from homonim_amd import CRS, RasterFuse, _hk
from homonim_amd.fuse import BlockCall, group_block_calls, shard
from homonim_amd.geo import Affine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('hk_fill_planes_dev', 'hk_boundless_window_dev')


# -- 1: the switch and the refusals -------------------------------------------------------------------------------------------------
def test_resident_is_off_by_default_and_kept_when_set():
    assert RasterFuse.create_device_config()['resident'] is False
    assert RasterFuse.create_device_config(resident=True)['resident'] is True
    assert RasterFuse.create_device_config(resident=1)['resident'] is True


@pytest.fixture
def no_library(monkeypatch):
    """ every way to a context fails: the refusals below are raised before any library call """
    def touched(*a, **kw):
        raise AssertionError('a context was asked for')
    for name in ('get_context', 'default_context', 'Context', 'load_library'):
        monkeypatch.setattr(_hk, name, touched)


def _two_grids():
    case = pb.CASES['3x-ref']
    src, ref = pb.closed_form_pair('3x-ref')
    return RasterFuse(src, ref, proc_crs='ref', crs=CRS(), transform=case.src_tf, ref_transform=case.ref_tf)


def test_a_shared_grid_is_refused_before_any_library_call(no_library):
    a = np.ones((1, 40, 50), np.float32)
    rf = RasterFuse(a, a.copy(), crs=CRS(), transform=Affine(10., 0., 0., 0., -10., 0.))
    with pytest.raises(ValueError, match='different grids.*one fused kernel per block'):
        rf.process(device_config=dict(resident=True))
    with pytest.raises(ValueError, match='SrcSpaceModel with mask_partial has no device-resident form'):
        rf.process(device_config=dict(resident=True), model_config=dict(mask_partial=True))


@pytest.mark.parametrize('config, named', [(dict(devices=[0, 1]), r'devices=\[0, 1\]'), (dict(devices=[0, 0]), r'devices=\[0, 0\]'),
                                            (dict(separate_contexts=True), 'separate_contexts=True')])
def test_two_devices_and_separate_contexts_are_refused_before_any_library_call(no_library, config, named):
    rf = _two_grids()
    with pytest.raises(ValueError, match='one device and one context: the resident rasters live on one device.*' + named):
        rf.process(device_config=dict(config, resident=True))


def test_without_the_switch_the_refusals_do_not_apply(no_library):
    """ the default route is reached (and here stopped at its first library call) """
    with pytest.raises(AssertionError, match='a context was asked for'):
        _two_grids().process(device_config=dict(devices=[0, 1]))


# -- 2: the grouping ----------------------------------------------------------------------------------------------------------------
def _windows(x):
    return (x.src_in_block, x.ref_in_block, x.src_out_block, x.ref_out_block)


@pytest.mark.parametrize('contiguous', [False, True], ids=['round-robin', 'contiguous'])
@pytest.mark.parametrize('world_size', [1, 2])
@pytest.mark.parametrize('n_bands', [1, 3])
@pytest.mark.parametrize('case_name', list(pb.CASES))
def test_the_calls_of_a_shard_hold_every_pair_once_in_runs_of_consecutive_bands(case_name, n_bands, world_size, contiguous):
    bps = pb.blocks_of(pb.CASES[case_name], n_bands, (1, 1), pb.block_mem(case_name, (1, 1)))
    seen_runs = set()
    for rank in range(world_size):
        own = shard(bps, rank, world_size, contiguous)
        calls = group_block_calls(own)
        assert all(isinstance(c, BlockCall) and c.n_bands >= 1 for c in calls)
        pairs = [(b, _windows(c)) for c in calls for b in c.bands]
        assert len(pairs) == len(set(pairs)) == len(own), 'a (band, block) pair is in two calls, or in none'
        assert set(pairs) == {(bp.band_i, _windows(bp)) for bp in own}
        for c in calls:
            assert list(c.bands) == list(range(c.band_i, c.band_i + c.n_bands))
            # a run is maximal: the band before it and the band after it are not of this shard's group
            assert (c.band_i - 1, _windows(c)) not in set(pairs) and (c.band_i + c.n_bands, _windows(c)) not in set(pairs)
            seen_runs.add(c.n_bands)
        if world_size == 1:
            assert len(calls) == len(bps) // n_bands and all(c.n_bands == n_bands for c in calls)
            assert [_windows(c) for c in calls] == [_windows(bp) for bp in bps if bp.band_i == 0], 'not in block order'
        assert group_block_calls(list(own)) == calls and own == shard(bps, rank, world_size, contiguous), 'not a pure function'
    if n_bands == 3 and world_size == 2 and contiguous:
        assert 2 in seen_runs, 'the contiguous shards of three bands hold runs of two'


def test_bands_that_are_not_consecutive_are_separate_calls():
    bps = pb.blocks_of(pb.CASES['3x-ref'], 4, (1, 1), pb.block_mem('3x-ref', (1, 1)))
    first = _windows(bps[0])
    own = [bp for bp in bps if _windows(bp) == first and bp.band_i in (0, 1, 3)]
    calls = group_block_calls(own)
    assert [(c.band_i, c.n_bands) for c in calls] == [(0, 2), (3, 1)]
    assert group_block_calls([]) == []


# -- 3: the entries -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    return _hk.load_library()


def test_the_entries_are_exported_declared_and_listed(lib):
    header = open(os.path.join(REPO, 'include', 'homonim_hk.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    text = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    for name in NEW_ENTRIES + ('hk_dev_mem_info',):
        assert hasattr(lib, name) and name in _hk.SIGNATURES
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), f'{name} is not declared in homonim_hk.h'
        assert re.search(r'^\| `' + name + r'`', text, flags=re.M), f'{name} has no row in INTEGRATION.md'
    assert lib.hk_abi_version() == 12 == _hk.ABI_VERSION


def _c_args(name):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'homonim_hk.h')).read(), flags=re.S)
    decl = re.search(r'\bint\s+' + name + r'\s*\((.*?)\)\s*;', header, flags=re.S).group(1)
    return [' '.join(a.split()) for a in decl.split(',')]


C_TYPES = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double}


@pytest.mark.parametrize('name', NEW_ENTRIES)
def test_the_argument_types_mirror_the_header(name):
    restype, argtypes = _hk.SIGNATURES[name]
    args = _c_args(name)
    assert restype is ctypes.c_int and len(args) == len(argtypes)
    for decl, t in zip(args, argtypes):
        if '*' in decl:
            assert t is ctypes.c_void_p, decl
        else:
            assert t is C_TYPES[decl.split()[0]], decl
    # the layout the issue names: planes, dtype, bands, shape, strides, then the value / the window and the output, the stream last
    names = [a.split()[-1].lstrip('*') for a in args]
    if name == 'hk_fill_planes_dev':
        assert names == ['ctx', 'planes_dev', 'dtype', 'n_bands', 'height', 'width', 'stride', 'band_stride', 'value', 'stream']
    else:
        assert names == ['ctx', 'planes_dev', 'dtype', 'n_bands', 'height', 'width', 'stride', 'band_stride', 'row_off', 'col_off',
                         'out_height', 'out_width', 'nodata_mode', 'nodata', 'out_dev', 'out_stride', 'out_band_stride', 'stream']


def test_a_null_context_is_the_argument_error(lib):
    assert lib.hk_fill_planes_dev(None, 0x1000, 1, 1, 4, 4, 4, 16, 0.0, 0) == _hk.HK_ERR_ARG
    assert b'ctx is NULL' in lib.hk_last_error()
    assert lib.hk_boundless_window_dev(None, 0x1000, 1, 1, 4, 4, 4, 16, -1, -1, 6, 6, 2, 0.0, 0x2000, 6, 36, 0) == _hk.HK_ERR_ARG
    assert b'ctx is NULL' in lib.hk_last_error()
    assert lib.hk_dev_mem_info(None, None, None) == _hk.HK_ERR_ARG


def test_the_fourteen_builds_are_on_the_ledger():
    names = sorted(b for b in _hk.build_ledger() if 'fill_planes_kernel' in b or 'boundless_window_kernel' in b)
    types = ('double', 'float', 'int', 'short', 'unsigned char', 'unsigned int', 'unsigned short')
    assert names == [f'boundless_window_kernel<{t}>' for t in types] + [f'fill_planes_kernel<{t}>' for t in types]


def test_window_helpers_clip_as_put_clips():
    from homonim_amd.geo import Window
    from homonim_amd.resident import clip_window, window_inside
    assert clip_window(Window(-2, -3, 10, 9), 5, 6) == (0, 0, 5, 6)
    assert clip_window(Window(4, 1, 10, 2), 5, 6) == (1, 4, 3, 6)
    r0, c0, r1, c1 = clip_window(Window(7, 0, 3, 3), 5, 6)
    assert c1 <= c0                                   # misses the raster
    assert window_inside(Window(0, 0, 6, 5), 5, 6) and not window_inside(Window(0, 0, 7, 5), 5, 6)
    assert not window_inside(Window(-1, 0, 3, 3), 5, 6)
