""" hk_srcspace_fit_apply (ABI version 11) without a GPU: the entry point and its descriptor, and the bit-identity argument of its
footprint kernel (hk_resample.hip footprint_typed_kernel) where it can be checked without a device.

That kernel reads the typed reference pixels under a destination pixel's footprint ONCE and forms two results from one loop: the
`average` value, and the coverage fraction of the valid mask that `mask_partial` needs.  Before it, the block made one pass to cast
the pixels to float32, one to average them, one to write a 0/1 valid plane and one to average that.  The loop is restated here in
numpy, operation for operation, and held bit for bit to oracle_np.reproject of the cast plane (with its nodata) and of the 0/1
valid plane (without nodata). """
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, assert_same_f32
from homonim_amd import _hk
from oracle import oracle_np as onp


@pytest.fixture(scope='module')
def lib():
    from homonim_amd import build
    build.build_hip(verbose=False)
    return _hk.load_library()


def test_ctypes_mirror_of_the_srcspace_desc_has_the_compilers_layout(tmp_path):
    assert _hk.ABI_VERSION >= 11
    cname, cls = 'hk_srcspace_desc', _hk.SrcSpaceDesc
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
    assert (ctypes.sizeof(cls),) == seen['sizeof'] == (4 * 8 + 2 * 4,)
    for name, _ in cls._fields_:
        desc = getattr(cls, name)
        assert (desc.offset, desc.size) == seen[name], name


def test_library_exports_the_entry_point_and_refuses_a_null_context(lib):
    assert hasattr(lib, 'hk_srcspace_fit_apply') and 'hk_srcspace_fit_apply' in _hk.SIGNATURES
    assert lib.hk_abi_version() >= 11
    desc = _hk.make_desc('gain', (3, 3), False, None, None, None)
    space = _hk.SrcSpaceDesc((3., 0., 3., 0.), 5, 0)
    src, ref, corr = np.zeros((4, 4), np.float32), np.zeros((12, 12), np.float32), np.zeros((4, 4), np.float32)
    vp = ctypes.c_void_p
    rc = lib.hk_srcspace_fit_apply(None, ctypes.byref(desc), None, ctypes.byref(space), src.ctypes.data_as(vp), 4, 4, 4,
                                   ref.ctypes.data_as(vp), 12, 12, 12, None, 2, corr.ctypes.data_as(vp), None)
    assert rc == _hk.HK_ERR_ARG
    assert lib.hk_last_error() == b'ctx is NULL'


# -- the one-pass loop ------------------------------------------------------------------------------------------------------------
def _footprint_axis(e0, e1, n):
    """ rs_footprint_axis of hk_resample_taps.h """
    p0, p1 = max(e0, 0.0), min(e1, float(n))
    i0, i1 = int(math.floor(p0 + 1e-10)), int(math.ceil(p1 - 1e-10))
    if i0 == i1 and i1 < n:
        i1 += 1
    return (i1 > i0 and i0 >= 0 and p1 > p0), p0, p1, i0, i1


def _edge_weight(p0, p1, i0, i1, p):
    """ rs_edge_weight """
    if i0 + 1 == i1:
        return 1.0
    return 1.0 - (p0 - i0) if p == i0 else (1.0 - (i1 - p1) if p == i1 - 1 else 1.0)


def _one_pass(typed, nodata, mapping, dst_shape):
    """ footprint_typed_kernel: value and coverage of every destination pixel from one loop over the typed pixels """
    kx, ox, ky, oy = mapping
    sh, sw = typed.shape
    value = np.full(dst_shape, np.nan, np.float32)
    cover = np.zeros(dst_shape, np.float32)
    nd = None if nodata is None else np.float32(nodata)
    for i in range(dst_shape[0]):
        rows, y0, y1, iy0, iy1 = _footprint_axis(ky * i + oy, ky * (i + 1) + oy, sh)
        for j in range(dst_shape[1]):
            cols, x0, x1, ix0, ix1 = _footprint_axis(kx * j + ox, kx * (j + 1) + ox, sw)
            tot = wsum = wall = 0.0
            if rows and cols:
                for yy in range(iy0, iy1):
                    wy = _edge_weight(y0, y1, iy0, iy1, yy)
                    for xx in range(ix0, ix1):
                        v = np.float32(typed[yy, xx])          # the conversion of cast_in_kernel, in registers
                        wgt = _edge_weight(x0, x1, ix0, ix1, xx) * wy
                        wall += wgt                             # every pixel of the clipped footprint
                        valid = True if nd is None else (not np.isnan(v) if np.isnan(nd) else not v == nd)
                        if not valid:
                            continue                            # (adds w * 0.0 to the coverage sum: no bit changes)
                        tot += float(v) * wgt
                        wsum += wgt                             # == the sum of w * 1.0 over the valid pixels
            if wsum > 0.0:
                value[i, j] = np.float32(tot / wsum)
            if wall > 0.0:
                cover[i, j] = np.float32(wsum / wall)
    return value, cover


def _typed_plane(nodata):
    rng = np.random.default_rng(5)
    if nodata is not None and np.isnan(nodata):
        a = rng.uniform(0., 4000., (7, 11)).astype(np.float32)
        a[0, :3] = np.nan            # one footprint entirely invalid (rows 0-1 x cols 0-2 below)
        a[1, :3] = np.nan
        a[3:5, 4] = np.nan
        a[6, 9:] = np.nan
        return a
    a = rng.integers(1, 4000, (7, 11)).astype(np.uint16)
    if nodata is not None:
        a[0, :3] = a[1, :3] = nodata
        a[3:5, 4] = nodata
        a[6, 9:] = nodata
    return a


@pytest.mark.parametrize('nodata', [float('nan'), 0., None], ids=['nan', 'numeric', 'none'])
@pytest.mark.parametrize('mapping', [(3.1, -0.7, 2.7, -0.9), (2.75, 0.0, 2.3333333333333335, 0.0), (3.1, 9.5, 2.7, -0.9)],
                         ids=['overhang', 'fractional', 'last-column-outside'])
def test_one_pass_value_and_coverage_equal_the_two_pass_chain(nodata, mapping):
    """ 7 x 11 -> 3 x 4 with fractional factors; 'overhang' leaves the first and last footprints of both axes partly outside the
    plane, 'last-column-outside' has footprints that share no area with it (fill: NaN value, coverage 0). """
    typed = _typed_plane(nodata)
    cast = typed.astype(np.float32)                      # launch_cast_in
    value, cover = _one_pass(typed, nodata, mapping, (3, 4))
    assert_same_f32(value, onp.reproject(cast, nodata, mapping, (3, 4), dst_nodata=np.nan, resampling='average'), 'value')
    valid = onp.mask_of(cast, nodata).astype(np.float32)  # launch_valid_plane
    assert_same_f32(cover, onp.reproject(valid, None, mapping, (3, 4), dst_nodata=None, resampling='average'), 'coverage')
    if mapping[1] < 0 and nodata is not None:
        assert np.isnan(value[0, 0]) and cover[0, 0] == 0          # the footprint without a valid pixel
        assert 0 < cover[1, 1] < 1 and not np.isnan(value[1, 1])   # ... and a partly valid one
    if mapping[1] > 9:
        assert np.isnan(value[:, 1:]).all() and (cover[:, 1:] == 0).all()
