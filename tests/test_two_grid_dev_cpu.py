""" The device-resident two-grid entries (hk_refspace_fit_apply_dev, hk_srcspace_fit_apply_dev) as far as they go without a GPU:
the layout of hk_two_grid_job, the two scratch-size helpers (plain host arithmetic) and the refusal of a NULL context. """
import ctypes
import os
import re
import subprocess

import pytest

from homonim_amd import _hk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    return _hk.load_library()


def test_two_grid_job_has_the_offsets_the_c_compiler_gives_the_header(tmp_path):
    """ Field by field, as tests/test_abi_cpu.py holds the other mirrors: offsetof() / sizeof() of hk_two_grid_job under gcc against
    _hk.TwoGridJob, and no field of the header that the mirror lacks. """
    cname, cls = 'hk_two_grid_job', _hk.TwoGridJob
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "homonim_hk.h"', 'int main(void) {',
             f'    printf("sizeof %zu\\n", sizeof({cname}));']
    for field in cls._fields_:
        lines.append(f'    printf("{field[0]} %zu %zu\\n", offsetof({cname}, {field[0]}), sizeof((({cname}*)0)->{field[0]}));')
    lines += ['    return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), str(src), '-o', str(exe)], check=True)
    seen = {}
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split('\n'):
        parts = ln.split()
        if len(parts) == 2:
            seen['sizeof'] = int(parts[1])
        elif len(parts) == 3:
            seen[parts[0]] = (int(parts[1]), int(parts[2]))
    assert ctypes.sizeof(cls) == seen['sizeof']
    for field in cls._fields_:
        desc = getattr(cls, field[0])
        assert (desc.offset, desc.size) == seen[field[0]], field[0]
    header = open(os.path.join(REPO, 'include', 'homonim_hk.h')).read()
    body = re.search(r'typedef struct[^{]*\{([^}]*)\}\s*' + cname + ';', header).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = set()
    for decl in body.split(';'):
        if decl.strip():
            for part in decl.strip().split(','):
                names.add(part.strip().split()[-1].lstrip('*'))
    assert names == {f[0] for f in cls._fields_}


def _job(n_bands=3, sh=37, sw=261, rh=12, rw=87, src_stride=None, params=False, valid=False, src_dtype='float32'):
    """ a job whose pointers are made-up addresses (the helpers look at NULL-ness and alignment only) """
    raster = lambda addr, dtype, shape, stride=None: _hk.DeviceRaster(addr, dtype, shape, stride)   # noqa: E731
    src = raster(0x10000, src_dtype, (n_bands, sh, sw), src_stride)
    return (src, raster(0x20000, 'float32', (n_bands, rh, rw)), raster(0x30000, 'float32', (n_bands, sh, sw)),
            params, raster(0x50000, 'uint8', (n_bands, sh, sw)) if valid else None)


def _refspace(model='gain-blk-offset', up=3, mask_partial=False, **kw):
    src, ref, corr, params, valid = _job(**kw)
    desc = _hk.make_desc(model, (5, 5), False, None, float('nan'), float('nan'))
    if params:
        params = _hk.DeviceRaster(0x40000, 'float32', (2 * src.shape[0], *ref.shape[1:]))
    job = _hk.make_two_grid_job(src, ref, corr, params or None, valid)
    io = _hk.make_io_desc(src.dtype, ref.dtype, corr.dtype, None)
    sp = _hk.make_space_desc((3, 0, 3, 0), (1 / 3, 0, 1 / 3, 0), 5, up, mask_partial)
    return desc, io, sp, job


def _srcspace(model='gain-blk-offset', resampling=5, mask_partial=False, **kw):
    src, ref, corr, params, valid = _job(**kw)
    desc = _hk.make_desc(model, (5, 5), False, None, float('nan'), float('nan'))
    if params:
        params = _hk.DeviceRaster(0x40000, 'float32', (2 * src.shape[0], *src.shape[1:]))
    job = _hk.make_two_grid_job(src, ref, corr, params or None, valid)
    io = _hk.make_io_desc(src.dtype, ref.dtype, corr.dtype, None)
    return desc, io, _hk.make_srcspace_desc((1 / 3, 0, 1 / 3, 0), resampling, mask_partial), job


FAMILIES = {'refspace': (_refspace, _hk.refspace_dev_scratch_bytes, 'up'), 'srcspace': (_srcspace, _hk.srcspace_dev_scratch_bytes, 'resampling')}


def _bytes(family, **kw):
    make, helper, _ = FAMILIES[family]
    desc, io, sp, job = make(**kw)
    return helper(desc, sp, job, io)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_scratch_helper_gives_a_multiple_of_256_for_a_valid_job(lib, family):
    n = _bytes(family)
    assert n > 0 and n % 256 == 0
    # one band's worth: the bands share it
    assert _bytes(family, n_bands=1) == n
    # the job's own scratch fields are not looked at
    make, helper, _ = FAMILIES[family]
    desc, io, sp, job = make()
    job.scratch, job.scratch_bytes = 0x1001, 1
    assert helper(desc, sp, job, io) == n
    # ... and io may be NULL: float32 everywhere
    assert helper(desc, sp, job, None) == n


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_scratch_helper_returns_0_for_what_the_entry_refuses(lib, family):
    make, helper, method = FAMILIES[family]
    assert _bytes(family, n_bands=0) == 0
    assert _bytes(family, src_stride=260) == 0              # a stride below the width
    assert _bytes(family, **{method: 7}) == 0               # gauss: not built
    desc, io, sp, job = make()
    for null in ('src', 'ref', 'corr'):
        bad = _hk.TwoGridJob.from_buffer_copy(job)
        setattr(bad, null, None)
        assert helper(desc, sp, bad, io) == 0, null
    bad = _hk.TwoGridJob.from_buffer_copy(job)
    bad.out_row0, bad.out_col0, bad.out_rows, bad.out_cols = 30, 0, 8, 10   # a window outside the block
    assert helper(desc, sp, bad, io) == 0
    bad = _hk.TwoGridJob.from_buffer_copy(job)
    bad.src_band_stride = 100                               # planes that overlap
    assert helper(desc, sp, bad, io) == 0
    bad = _hk.TwoGridJob.from_buffer_copy(job)
    bad.reserved = 1
    assert helper(desc, sp, bad, io) == 0


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_scratch_helper_does_not_shrink_when_more_is_asked_for(lib, family):
    base = _bytes(family)
    assert _bytes(family, src_dtype='uint8') >= base
    assert _bytes(family, src_dtype='uint8') > base         # the raw plane of a typed input is part of the slab
    assert _bytes(family, mask_partial=True) > base
    assert _bytes(family, valid=True) > base
    assert _bytes(family, params=True) >= base


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_a_null_context_is_the_argument_error(lib, family):
    make, _, _ = FAMILIES[family]
    desc, io, sp, job = make()
    entry = lib.hk_refspace_fit_apply_dev if family == 'refspace' else lib.hk_srcspace_fit_apply_dev
    assert entry(None, ctypes.byref(desc), ctypes.byref(io), ctypes.byref(sp), ctypes.byref(job), None) == _hk.HK_ERR_ARG
    assert b'ctx is NULL' in lib.hk_last_error()
    assert lib.hk_abi_version() == 12


def check_model_refusals():
    """ RefSpaceModel.fit_apply_dev / SrcSpaceModel.fit_apply_dev refuse, before any device call: two CRSs and rotated grids in
    fit_apply's words, grids of opposite orientation (a device raster is not flipped for the caller), and a shared grid, which
    hk_fit_apply_dev already serves.  (tests/test_gpu_two_grid_dev.py runs it as well.) """
    import numpy as np
    from homonim_amd import Affine, CRS, Model, RasterArray, RefSpaceModel, SrcSpaceModel
    tm25, utm35s = CRS('x [1024=1; 2048=4326; 3075=1; 3080=25.0]'), CRS('EPSG:32735')
    fine, coarse = Affine(10., 0., 500., 0., -10., 9000.), Affine(30., 0., 500., 0., -30., 9000.)

    def raster(shape, transform, crs=utm35s, addr=0x10000):
        return _hk.DeviceRaster(addr, 'float32', shape, transform=transform, crs=crs, nodata=float('nan'))

    src, corr = raster((1, 36, 36), fine), _hk.DeviceRaster(0x30000, 'float32', (1, 36, 36))
    for model in (RefSpaceModel(Model.gain, (3, 3)), SrcSpaceModel(Model.gain, (3, 3))):
        # the words are fit_apply's own
        a = RasterArray(np.ones((36, 36), np.float32), utm35s, fine)
        for other_crs, other_transform, match in ((tm25, coarse, r'reproject\(crs='), (utm35s, Affine(30., 5., 500., 5., -30., 9000.), 'rotated')):
            with pytest.raises(NotImplementedError, match=match) as host:
                model.fit_apply(a, RasterArray(np.ones((12, 12), np.float32), other_crs, other_transform))
            with pytest.raises(NotImplementedError, match=match) as dev:
                model.fit_apply_dev(src, raster((1, 12, 12), other_transform, other_crs, 0x20000), corr)
            assert str(dev.value) == str(host.value)
        with pytest.raises(ValueError, match='a device raster is not flipped for the caller'):
            model.fit_apply_dev(src, raster((1, 12, 12), Affine(30., 0., 500., 0., 30., 8640.), addr=0x20000), corr)
        with pytest.raises(ValueError, match='needs its `transform`'):
            model.fit_apply_dev(src, _hk.DeviceRaster(0x20000, 'float32', (1, 12, 12)), corr)
        with pytest.raises(ValueError, match='hk_fit_apply_dev'):
            model.fit_apply_dev(src, raster((1, 36, 36), fine, addr=0x20000), corr)


def test_model_fit_apply_dev_refusals_need_no_device():
    check_model_refusals()
