""" The structs the warp entry points take -- hk_crs_desc, hk_warp_desc -- field by field against offsetof() / sizeof() of
include/homonim_hk.h as gcc lays them out, like tests/test_abi_cpu.py does for the other structs; and the descriptor
``_hk.make_warp_desc`` fills in from CRS definitions and geo-transforms. """
import ctypes
import os
import subprocess

import pytest

from conftest import REPO
from homonim_amd import Affine, CRS, _hk, crs


def test_ctypes_mirrors_of_the_warp_structs_have_the_compilers_layout(tmp_path):
    pairs = [('hk_crs_desc', _hk.CrsDesc), ('hk_warp_desc', _hk.WarpDesc)]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "homonim_hk.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'    printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for name, _ in cls._fields_:
            lines.append(f'    printf("{cname} {name} %zu %zu\\n", offsetof({cname}, {name}), sizeof((({cname}*)0)->{name}));')
    lines += ['    return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), str(src), '-o', str(exe)],
                   check=True)
    seen = {}
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        parts = ln.split()
        seen[(parts[0], parts[1])] = tuple(int(v) for v in parts[2:])
    for cname, cls in pairs:
        assert (ctypes.sizeof(cls),) == seen[(cname, 'sizeof')], cname
        for name, _ in cls._fields_:
            desc = getattr(cls, name)
            assert (desc.offset, desc.size) == seen[(cname, name)], f'{cname}.{name}'
    assert ctypes.sizeof(_hk.CrsDesc) == 8 + 7 * 8 and ctypes.sizeof(_hk.WarpDesc) == 2 * 64 + 8 * 8
    assert _hk.ABI_VERSION >= 9


def test_make_warp_desc():
    tm, utm = crs.parse(CRS('x [1024=1; 2048=4326; 3075=1; 3080=25.0]')), crs.parse(CRS('EPSG:32735'))
    w = _hk.make_warp_desc(tm, Affine(30., 0., -60390., 0., -30., -3722700.), utm, Affine(5., 0., 254000., 0., -5., 6278000.))
    assert (w.src_crs.kind, w.src_crs.a, w.src_crs.inv_f, w.src_crs.lon0, w.src_crs.k0) == (1, 6378137.0, 298.257223563, 25., 1.)
    assert (w.dst_crs.lon0, w.dst_crs.k0, w.dst_crs.fe, w.dst_crs.fn) == (27., 0.9996, 500000., 10000000.)
    assert list(w.src_gt) == [-60390., 30., -3722700., -30.] and list(w.dst_gt) == [254000., 5., 6278000., -5.]
    with pytest.raises(NotImplementedError, match='rotated'):
        _hk.make_warp_desc(tm, Affine(30., 1., 0., 0., -30., 0.), utm, Affine.identity())
