""" The workspace layouts of the in-painting and of the block statistics (homonim_amd/csrc/hk_layout.h), without a GPU: the header is
plain C++, so a stand-alone program (tests/c/inpaint_layout_host.cpp, which states the checks) walks it under AddressSanitizer +
UBSan -- order, alignment, the bytes each kernel indexes, the total, and what the library reserved before the layouts were one
function each. """
import os
import subprocess

from conftest import REPO


def test_the_workspace_layouts_as_a_stand_alone_program_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / 'inpaint_layout_host_san'
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(REPO, 'homonim_amd', 'csrc'), os.path.join(REPO, 'tests', 'c', 'inpaint_layout_host.cpp'),
                    '-o', str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and not res.stderr, res.stderr[-3000:]
    assert res.stdout.split('\n')[:-1] == ['inpaint_layout: 84 shapes', 'norm_layout: 4 shapes']
