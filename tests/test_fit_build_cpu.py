"""
The chooser of the fused kernel's build never asks for a build that does not exist (no GPU: `hk_debug_fit_build` is host arithmetic,
and the ledger's records are on their list from the moment the library is loaded).

`hk::choose_fit_build` (csrc/hk_kernels.hip) turns a launch -- model, kernel shape, nodata, the planes it is handed, the phase, the
testing switches -- into one instantiation of the kernel template; `hk::fit_build_exists` (csrc/hk_kernels.h) states which are
instantiated, and the table of csrc/hk_fit_kernel.h instantiates exactly those.  The sweep walks every model x R2 set x threshold,
every odd kernel height up to 41 and 63, 65, 127, 129, 255 (either side of every threshold of `fill_args` and of the 64 KiB LDS
step), every odd width up to 41 and the widest admitted, the plane sets the entry points produce and the forced rings.  The
product of the remaining switches is trimmed, not the shapes: the nine nodata pairs and force-general, which only decide dense or
general, rotate through that inner product (18 values, 71 steps per shape), so that every (planes, ring) pair meets each of
them at every 18th shape.
"""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

from homonim_amd import _hk

KHS = tuple(range(1, 42, 2)) + (63, 65, 127, 129, 255)
KW_MAX = 2 * (4 * 24) + 1   # overlap_lanes_for(kw // 2) = ceil(kw // 2 / 4) <= 24 (validate_desc)
KWS = tuple(range(1, 42, 2)) + (KW_MAX,)
NODATA = (None, np.nan, -3.0)
RINGS = (None, 0, 1, 2, 3)
# (planes, phase): what the entry points hand a launch
PARAMS = ('gain', 'offset', 'corr', 'fail_count')
LAUNCHES = (
    (PARAMS, 0),                                              # parameters out (the R2 plane is added where R2 is asked for)
    (('corr',), 0),                                           # corrected only, device job without a counter
    (('corr', 'fail_count'), 0), (('corr', 'fail_count'), 1), (('corr', 'fail_count'), 2),   # ... with one: the three phases
    (('corr', 'fail_count', 'offset', 'flags'), 0),           # ... leaving the in-painting's inputs (job scratch)
    (('offset', 'flags'), 0),                                 # the in-painting's inputs alone
    (('corr', 'offset_in'), 0), (('gain', 'offset', 'corr', 'offset_in'), 0),                # closing pass
    (('corr', 'offset_in', 'flags'), 0), (('gain', 'offset', 'corr', 'offset_in', 'flags'), 0),
    (('corr', 'jobs'), 0), (('gain', 'offset', 'corr', 'jobs'), 0), (('corr', 'fail_count', 'jobs'), 1),   # job table
)


@pytest.fixture(scope='module')
def asked():
    """ ask(desc, planes, phase, ring, general) -> the build's ledger name, or None where the entry refuses the launch (HK_ERR_ARG) """
    lib = _hk.load_library()
    name = C.create_string_buffer(88)

    def ask(desc, planes, phase, ring, general):
        rc = lib.hk_debug_fit_build(C.byref(desc), 44, 300, 1, planes, phase, -1 if ring is None else ring, int(general), name, 88)
        assert rc in (_hk.HK_OK, _hk.HK_ERR_ARG), rc
        return name.value.decode() if rc == _hk.HK_OK else None
    return ask


def _bits(planes, find_r2):
    return sum(_hk.FIT_PLANES[p] for p in planes) | (_hk.FIT_PLANES['r2'] if find_r2 and planes is PARAMS else 0)


def test_every_chosen_build_is_in_the_ledger(asked):
    ledger = set(_hk.build_ledger())
    assert sum(n.startswith('fit_') for n in ledger) == 424
    switches = itertools.cycle(itertools.product(itertools.product(NODATA, NODATA), (False, True)))
    n_asked = 0
    for model, find_r2, thresh in itertools.product(_hk.MODEL_CODES, (False, True), (None, 0.25)):
        def what():   # (for the message of a failing assertion)
            return model, find_r2, thresh, kh, kw, planes, phase, ring, src_nd, ref_nd, general
        desc = _hk.make_desc(model, (1, 1), find_r2, thresh, None, None)
        r2_mask = model == 'gain-offset' and thresh is not None
        batch = model == 'gain-blk-offset' and not find_r2           # fit_batch_build
        for kh, kw in itertools.product(KHS, KWS):
            if model == 'gain-offset' and kh * kw < 2:
                continue
            desc.kh, desc.kw = kh, kw
            next(switches)   # (71 steps per shape, prime to the 18 values: every launch meets every value over 18 shapes)
            for (planes, phase), ring in itertools.product(LAUNCHES, RINGS):
                (src_nd, ref_nd), general = next(switches)
                (desc.src_nodata_mode, desc.src_nodata), (desc.ref_nodata_mode, desc.ref_nodata) = _hk.nodata_code(src_nd), _hk.nodata_code(ref_nd)
                got = asked(desc, _bits(planes, find_r2), phase, ring, general)
                n_asked += 1
                if got is not None:
                    assert got in ledger, (what(), got)
                if 'jobs' in planes:
                    # a request the launch table used to answer with hipErrorInvalidValue is refused, not chosen
                    assert (got is not None) == (batch and phase == 0), (what(), got)
                    assert got is None or got.endswith(',1>'), (what(), got)
                elif phase == 0:
                    assert got is not None, what()
                    dense = src_nd is None and ref_nd is None and not general and model != 'gain-blk-offset'
                    m = re.fullmatch(r'fit_apply_kernel<(\d),(\d),(-?\d),(\d),(\d),0,(\d),0>', got)
                    assert m, (what(), got)
                    with_r2 = (find_r2 or r2_mask) and 'offset_in' not in planes
                    assert (int(m[1]), int(m[2]), int(m[4])) == (_hk.MODEL_CODES[model], int(with_r2), int(dense)), (what(), got)
                if planes == ('corr', 'fail_count') and phase == 0:
                    # the certificate and the list launch are chosen only where BOTH builds exist -- gain-offset with the r2 mask on
                    # the full or the centre ring, window counts below 2^16 -- and then for the complete build's own shape
                    rw, d, rg = m[3], m[4], int(m[5])
                    cert, lst = asked(desc, _bits(planes, find_r2), 1, ring, general), asked(desc, _bits(planes, find_r2), 2, ring, general)
                    if r2_mask and rg in (1, 2) and kh * kw <= 65535:
                        assert cert == f'fit_apply_kernel<2,1,{rw},{d},{rg},1,1,0>' and lst == f'fit_list_kernel<2,1,{rw},{d},{rg}>', (what(), cert, lst)
                        assert cert in ledger and lst in ledger, what()
                    else:
                        assert cert is None and lst is None, (what(), cert, lst)
                elif phase and planes != ('corr', 'fail_count'):
                    assert got is None, (what(), got)
    assert n_asked > 400000


def test_certificate_and_list_are_refused_where_other_planes_are_written(asked):
    """ R2, gain, the in-painting's flags or in-painted offsets in the launch: the certificate build has no registers for them """
    desc = _hk.make_desc('gain-offset', (5, 5), False, 0.25, np.nan, np.nan)
    base = _hk.FIT_PLANES['corr'] | _hk.FIT_PLANES['fail_count']
    for phase in (1, 2):
        assert asked(desc, base, phase, None, False) is not None
        assert asked(desc, _hk.FIT_PLANES['corr'], phase, None, False) is None   # failures not counted
        for extra in ('gain', 'r2', 'flags', 'offset_in', 'jobs'):
            assert asked(desc, base | _hk.FIT_PLANES[extra], phase, None, False) is None, (phase, extra)
    with pytest.raises(ValueError):
        _hk.fit_build(desc, (1, 44, 300), ('corr', 'fail_count', 'gain'), phase=1)
    assert _hk.fit_build(desc, (1, 44, 300), ('corr', 'fail_count'), phase=2) == 'fit_list_kernel<2,1,2,0,1>'
