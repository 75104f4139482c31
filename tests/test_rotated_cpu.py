""" Rotated and sheared rasters, the parts that need no GPU: ``Affine.rotation``; the layout of hk_affine_warp_desc and the
descriptor ``_hk.make_affine_warp_desc`` fills; the GeoTIFF round trip of a rotated geo-transform (and the unchanged bytes of a
north-up file); ``geo.suggested_warp_grid`` within one CRS and ``warp_scale`` through full affines; the numpy statement of the
device's coordinate expressions against exact rational arithmetic (tests/_rotated_grids.py states the bar); what stays refused. """
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import _rotated_grids as rg
from conftest import GOLDEN_DIR, REPO
from homonim_amd import Affine, CRS, Model, RasterArray, RefSpaceModel, _hk, crs
from homonim_amd.errors import IoError
from homonim_amd.geo import grid_mapping, suggested_warp_grid
from homonim_amd.raster_array import warp_scale
from homonim_amd.tiff import read_tiff, write_tiff

UTM35S, WEB = CRS('EPSG:32735'), CRS('EPSG:3857')


# -- 1. Affine.rotation ---------------------------------------------------------------------------------------------------------------
def test_rotation_is_exact_at_quarter_turns_and_inverts():
    assert Affine.rotation(0.) == Affine(1., 0., 0., 0., 1., 0.)
    assert Affine.rotation(90.) == Affine(0., -1., 0., 1., 0., 0.)
    assert Affine.rotation(180.) == Affine(-1., 0., 0., 0., -1., 0.)
    assert Affine.rotation(270.) == Affine(0., 1., 0., -1., 0., 0.) == Affine.rotation(-90.)
    assert Affine.rotation(450.) == Affine.rotation(90.)
    r = Affine.rotation(30.)
    assert r.a == r.e == math.cos(math.radians(30.)) and r.d == -r.b == math.sin(math.radians(30.))
    a, b = Affine.translation(254000., 6278000.) * Affine.rotation(30.), Affine.scale(5., -5.) * Affine(1., 0.1, 3., 0., 1., -7.)
    for x, y in ((0., 0.), (17.5, -3.25), (-1e3, 2e3)):
        bx, by = (~(a * b)) * ((a * b) * (x, y))
        assert abs(bx - x) < 1e-6 and abs(by - y) < 1e-6
    # the transform of the reference's rotated fixtures (tests/conftest.py:378-517 there)
    assert Affine(1., 0., 0., 0., -1., 0.) * Affine.rotation(90.) * Affine.translation(5., -15.) == Affine(0., -1., 15., -1., 0., -5.)


# -- 2. ABI -------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_of_the_affine_warp_desc_has_the_compilers_layout(tmp_path):
    cname, cls = 'hk_affine_warp_desc', _hk.AffineWarpDesc
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "homonim_hk.h"', 'int main(void) {',
             f'    printf("sizeof %zu\\n", sizeof({cname}));']
    for name, _ in cls._fields_:
        lines.append(f'    printf("{name} %zu %zu\\n", offsetof({cname}, {name}), sizeof((({cname}*)0)->{name}));')
    lines += ['    return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), str(src), '-o', str(exe)],
                   check=True)
    seen = {}
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        parts = ln.split()
        seen[parts[0]] = tuple(int(v) for v in parts[1:])
    assert (ctypes.sizeof(cls),) == seen['sizeof'] == (2 * 64 + 8 + 12 * 8,)
    for name, _ in cls._fields_:
        desc = getattr(cls, name)
        assert (desc.offset, desc.size) == seen[name], name
    assert _hk.ABI_VERSION >= 10
    assert ctypes.sizeof(_hk.WarpDesc) == 2 * 64 + 8 * 8        # hk_warp_desc keeps its layout


def test_make_affine_warp_desc():
    src_tf, dst_tf = rg.PAIRS['15deg-5m-from-minus40deg-south-up-30m']
    w = _hk.make_affine_warp_desc(None, src_tf, None, dst_tf)
    assert (w.same_crs, w.reserved) == (1, 0)
    assert tuple(w.src_gt) == tuple(src_tf) and tuple(w.dst_gt) == tuple(dst_tf)
    tm, utm = crs.parse(CRS('x [1024=1; 2048=4326; 3075=1; 3080=25.0]')), crs.parse(UTM35S)
    w = _hk.make_affine_warp_desc(tm, src_tf, utm, dst_tf)
    assert w.same_crs == 0 and tuple(w.src_gt) == tuple(src_tf) and tuple(w.dst_gt) == tuple(dst_tf)
    assert (w.src_crs.kind, w.src_crs.lon0, w.src_crs.k0) == (1, 25., 1.)
    assert (w.dst_crs.lon0, w.dst_crs.k0, w.dst_crs.fe, w.dst_crs.fn) == (27., 0.9996, 500000., 10000000.)
    with pytest.raises(ValueError, match='both'):
        _hk.make_affine_warp_desc(tm, src_tf, None, dst_tf)


# -- 3. GeoTIFF ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tf', [rg.rotated(254000., 6278000., 30., 5.), Affine(30., 3., 254000., -0.5, -30., 6278000.)],
                         ids=['rotated-30deg', 'sheared'])
def test_a_rotated_transform_survives_the_tiff_round_trip(tmp_path, tf):
    data = np.random.default_rng(3).uniform(0., 1., (2, 37, 53)).astype(np.float32)
    data[0, 4, 5] = np.nan
    fn = tmp_path / 'rotated.tif'
    with pytest.raises(IoError, match='rotated=True'):       # opt-in: the package's own outputs are north-up
        write_tiff(fn, data, tf, UTM35S, float('nan'))
    write_tiff(fn, data, tf, UTM35S, float('nan'), rotated=True)
    back = read_tiff(fn)
    assert tuple(back.transform) == tuple(tf)
    assert back.crs == UTM35S and math.isnan(back.nodata)
    assert np.array_equal(back.array, data, equal_nan=True)


def test_a_north_up_file_is_written_byte_for_byte_as_before(tmp_path):
    """ tests/golden/rotated/north_up_before_rotation.tif was written by this very call before ``write_tiff`` knew the
    ModelTransformation tag """
    rng = np.random.default_rng(11)
    data = rng.uniform(-1., 1., (3, 40, 70)).astype(np.float32)
    data[:, :3] = np.nan
    fn = tmp_path / 'north_up.tif'
    write_tiff(fn, data, Affine(5., 0., 254000., 0., -5., 6278000.), UTM35S, float('nan'), metadata={'FUSE_MODEL': 'gain-offset'},
               tile=32, descriptions=['r', None, 'b'])
    with open(fn, 'rb') as f, open(os.path.join(GOLDEN_DIR, 'rotated', 'north_up_before_rotation.tif'), 'rb') as g:
        assert f.read() == g.read()


# -- 4. grids -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('label', [UTM35S, WEB], ids=['utm', 'epsg3857'])
@pytest.mark.parametrize('pixel', [1.0, 0.5])
def test_the_suggested_grid_of_a_quarter_turn_is_the_unrotated_grid(label, pixel):
    """ a raster stored turned by 90 degrees: its outline is exact, ``hypot`` is symmetric and scales exactly by powers of two, so
    the pixel size, the extent and the shape come back exactly """
    h, w = 83, 271
    north_up = Affine(pixel, 0., 254000., 0., -pixel, 6278000.)
    # np.rot90(data) of an (h, w) north-up raster: rot[r, c] = data[c, w - 1 - r], i.e. column = w - stored row, row = stored column
    stored = north_up * Affine(0., -1., float(w), 1., 0., 0.)
    assert (stored.a, stored.e) == (0., 0.)
    tf, shape = suggested_warp_grid(label, stored, (w, h), label)
    assert shape == (h, w) and tuple(tf) == tuple(north_up)


def test_the_suggested_grid_of_a_30_degree_raster_is_its_bounding_box():
    h, w, pixel = 80, 120, 5.
    tf = rg.rotated(254000., 6278000., 30., pixel)
    out, (oh, ow) = suggested_warp_grid(WEB, tf, (h, w), WEB)
    xs, ys = zip(*(tf * p for p in ((0., 0.), (w, 0.), (w, h), (0., h))))
    assert (out.b, out.d) == (0., 0.) and out.e == -out.a
    assert abs(out.a - pixel) <= 1e-12 * pixel
    assert out.c == min(xs) and out.f == max(ys)
    assert (oh, ow) == (int((max(ys) - min(ys)) / out.a + 0.5), int((max(xs) - min(xs)) / out.a + 0.5))
    with pytest.raises(NotImplementedError):       # the mapping between two axis-aligned grids has no meaning here
        grid_mapping(tf, out)


def test_warp_scale_of_a_pure_rotation_is_one():
    for deg in (30., 90., -40., 77.):
        src_tf = rg.rotated(254000., 6278000., deg, 5.)
        kx, ky = warp_scale(WEB, Affine(5., 0., 253500., 0., -5., 6278400.), (83, 271), WEB, src_tf)
        assert abs(kx - 1.) < 1e-12 and abs(ky - 1.) < 1e-12
    kx, ky = warp_scale(WEB, Affine(15., 0., 253500., 0., -15., 6278400.), (30, 90), WEB, rg.rotated(254000., 6278000., 30., 5.))
    assert abs(kx - 3.) < 1e-11 and abs(ky - 3.) < 1e-11


# -- 5. coordinates -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', list(rg.PAIRS))
def test_the_affine_expressions_against_exact_rational_arithmetic(pair):
    src_tf, dst_tf = rg.PAIRS[pair]
    for what, shape, off in rg.LATTICES:
        gx, gy = rg.coords_np(src_tf, dst_tf, shape, off)
        err, bar = rg.max_error(pair, shape, off, gx, gy), rg.bar(pair, shape, off)
        print(f'[affine coords, numpy] {pair} {what}: largest error {err:.3e} source pixels, bar {bar:.3e} ({err / bar:.3f} of it)')
        assert err <= bar, f'{pair} {what}: {err} > {bar}'
        if pair == '90deg-1m':
            assert err == 0.


# -- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_what_stays_refused():
    tf = rg.rotated(254000., 6278000., 30., 5.)
    a = RasterArray(np.ones((8, 12), np.float32), UTM35S, tf)
    for mode in ('average', 'mode', 'max', 'min', 'med', 'q1', 'q3', 'sum', 'rms'):
        with pytest.raises(NotImplementedError, match=mode):
            a.reproject(transform=Affine(5., 0., 254000., 0., -5., 6278000.), shape=(8, 12), resampling=mode)
        with pytest.raises(NotImplementedError, match=mode):
            RasterArray(a.array, UTM35S, Affine(5., 0., 254000., 0., -5., 6278000.)).reproject(transform=tf, shape=(8, 12),
                                                                                               resampling=mode)
    b = RasterArray(np.ones((8, 12), np.float32), UTM35S, Affine(5., 0., 254000., 0., -5., 6278000.))
    with pytest.raises(NotImplementedError, match='rotated'):
        RefSpaceModel(Model.gain, (3, 3)).fit(a, b)
    tm, utm = crs.parse(CRS('x [1024=1; 2048=4326; 3075=1; 3080=25.0]')), crs.parse(UTM35S)
    with pytest.raises(NotImplementedError, match='rotated'):
        _hk.make_warp_desc(tm, tf, utm, Affine.identity())
