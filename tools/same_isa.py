""" Do two builds hold the same machine code?  The acceptance gate of a refactor that must not change what the compiler emits.

    python tools/same_isa.py DIR_A DIR_B

For every *.o present in both directories: the gfx950 code object is extracted (as tools/kernel_regs.py does), disassembled with
llvm-objdump -d and cut into symbols; per symbol the instruction text (encodings included, absolute addresses dropped) of A is
compared with B's as a whole -- nothing here knows about particular instructions.  The register / scratch / LDS figures of the
metadata notes are compared as well and printed for every kernel that differs.  (Two compiles of the same source give different
code-object BYTES -- hence disassembly.)  Exit status 1 on any difference, or when an object or a symbol exists on one side only. """
import os
import re
import subprocess
import sys
import tempfile

from kernel_regs import LLVM, demangle

FIGURES = ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'vgpr_spill_count', 'group_segment_fixed_size')


def code_object(obj, tmp):
    """ path of the gfx950 code object of `obj`, extracted into `tmp` """
    obj = os.path.abspath(obj)
    src_dir = os.path.dirname(obj)
    subprocess.run([f'{LLVM}/llvm-objdump', '--offloading', obj], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for f in os.listdir(src_dir):   # (some versions write the bundles beside the INPUT)
        if f.startswith(os.path.basename(obj) + '.0.'):
            os.replace(os.path.join(src_dir, f), os.path.join(tmp, f))
    cos = [f for f in os.listdir(tmp) if 'gfx950' in f]
    return os.path.join(tmp, cos[0]) if cos else None   # (None: a host-only object, hk_api.o)


def symbols(obj):
    """ {symbol: instruction text}, {kernel: figures line} of the gfx950 code object of `obj`; both empty for an object without one """
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        if co is None:
            return {}, {}
        dis = subprocess.run([f'{LLVM}/llvm-objdump', '-d', co], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([f'{LLVM}/llvm-readelf', '--notes', co], capture_output=True, text=True, check=True).stdout
    text, name = {}, None
    for line in dis.split('\n'):
        m = re.match(r'^[0-9a-fA-F]+ <(.+)>:$', line)
        if m:
            name = m.group(1)
            text[name] = []
        elif name is not None and line.strip():
            text[name].append(re.sub(r'//\s*[0-9A-Fa-f]+:', '//', line.strip()))   # the address of the instruction, not its encoding
    figures = {}
    for e in re.split(r'\n\s+- \.agpr_count', notes)[1:]:
        vals = [int(re.search(r'\.' + key + r':\s+(\d+)', e).group(1)) for key in FIGURES]
        figures[re.search(r'\.name:\s+(\S+)', e).group(1)] = 'vgpr %3d sgpr %3d scratch %4d B spilled %3d lds %5d B' % tuple(vals)
    return {k: '\n'.join(v) for k, v in text.items()}, figures


def compare(obj_a, obj_b):
    """ number of differences between two objects; prints one line per object and the details of every difference """
    (ta, fa), (tb, fb) = symbols(obj_a), symbols(obj_b)
    only = sorted(set(ta) ^ set(tb))
    differ = sorted(s for s in set(ta) & set(tb) if ta[s] != tb[s] or fa.get(s) != fb.get(s))
    verdict = 'identical' if not only and not differ else f'{len(differ)} DIFFERENT, {len(only)} on one side only'
    print(f'{os.path.basename(obj_a):24s} {len(ta):4d} symbols, {len(fa):4d} kernels: {verdict}')
    for s, n in zip(only, demangle(only)):
        print(f'    only in {"A" if s in ta else "B"}: {n}')
    for s, n in zip(differ, demangle(differ)):
        print(f'    differs: {n}')
        print(f'        A: {ta[s].count(chr(10)) + 1:6d} instructions  {fa.get(s, "")}')
        print(f'        B: {tb[s].count(chr(10)) + 1:6d} instructions  {fb.get(s, "")}')
    return len(only) + len(differ)


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    dir_a, dir_b = sys.argv[1:]
    objs = sorted(f for f in os.listdir(dir_a) if f.endswith('.o') and os.path.exists(os.path.join(dir_b, f)))
    if not objs:
        sys.exit(f'no *.o common to {dir_a} and {dir_b}')
    bad = sum(compare(os.path.join(dir_a, f), os.path.join(dir_b, f)) for f in objs)
    print('every kernel identical' if not bad else f'{bad} difference(s)')
    sys.exit(1 if bad else 0)
