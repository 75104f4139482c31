"""
The same builds as recorded, case by case: tests/golden/fit_build_choices.json (tools/record_fit_builds.py) holds, for every case of the
decision space of tests/test_gpu_build_sweep.py, which builds of the fused kernel the library launched and how often at the commit
named in the file.  A refactor of the selection (hk::choose_fit_build) must reproduce it exactly; a change of launch policy
re-records the file on purpose, and the diff of the JSON shows what moved.  No results are compared here (test_gpu_build_sweep.py
holds every one of these launches to the oracle).
"""
import json
import os

import pytest

import _fit_build_choices as fbc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fit_build_choices.json')


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as f:
        record = json.load(f)
    assert set(record['choices']) == {fbc.config_id(*c) for c in fbc.CONFIGS}
    return record['choices']


@pytest.mark.parametrize('model, find_r2, thresh, nodata', fbc.CONFIGS)
def test_every_case_launches_the_recorded_builds(recorded, model, find_r2, thresh, nodata):
    exp = recorded[fbc.config_id(model, find_r2, thresh, nodata)]
    got = fbc.choices((model, find_r2, thresh, nodata))
    assert got.keys() == exp.keys()
    moved = {case: (exp[case], got[case]) for case in exp if got[case] != exp[case]}
    assert not moved, f'{len(moved)} of {len(exp)} cases launch other builds than recorded, e.g. {list(moved.items())[:3]}'
    assert all(hits for hits in got.values())   # (every case launches the fused kernel)
