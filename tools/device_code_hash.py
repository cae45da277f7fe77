#!/usr/bin/env python3
"""Device code of the shipped build's objects (build/obj/*.o), for "this change moved no kernel":

  python tools/device_code_hash.py [objdir]             sha256 of the gfx950 .text section of every object
  python tools/device_code_hash.py --kernels [objdir]   per kernel: unit, size, sha256 of its bytes in .text, name
  python tools/device_code_hash.py --names [objdir]     per kernel: unit, name (the *.kd descriptors; tests/golden/kernel_set.txt)

Two trees whose per-kernel lines agree compile to the same kernels; the per-unit hash also covers the order they were
emitted in."""
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'
OBJ = os.path.join(ROOT, 'build', 'obj')


def _run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True).stdout


def unbundle(o, td):
    """The gfx950 code object of host object `o`, written into directory `td` (None: the object has no device code)."""
    fat, co = os.path.join(td, 'fat'), os.path.join(td, 'co')
    _run(LLVM + '/llvm-objcopy', '--dump-section', '.hip_fatbin=' + fat, o)
    if not os.path.exists(fat):
        return None
    _run(LLVM + '/clang-offload-bundler', '--unbundle', '--type=o', '--input=' + fat,
         '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co)
    return co if os.path.exists(co) and os.path.getsize(co) else None


def text_of(co, td):
    txt = os.path.join(td, 'text')
    _run(LLVM + '/llvm-objcopy', '--dump-section', '.text=' + txt, co)
    return open(txt, 'rb').read() if os.path.exists(txt) else None


def kernels_of(co, td):
    """[(mangled name, size, sha256 of the kernel's bytes)] of a code object, sorted by name: the functions that have a
    kernel descriptor (NAME.kd)."""
    text = text_of(co, td)
    if text is None:
        return []
    base = None
    for ln in _run(LLVM + '/llvm-readelf', '-SW', co).splitlines():
        f = ln.replace('[', ' ').replace(']', ' ').split()
        if len(f) > 3 and f[1] == '.text':
            base = int(f[3], 16)
    funcs, kds = {}, set()
    for ln in _run(LLVM + '/llvm-readelf', '-sW', co).splitlines():
        f = ln.split()
        if len(f) < 8 or not f[0].endswith(':') or not f[0][:-1].isdigit():
            continue
        value, size, typ, name = int(f[1], 16), int(f[2], 0), f[3], f[7]
        if name.endswith('.kd'):
            kds.add(name[:-3])
        elif typ == 'FUNC':
            funcs[name] = (value, size)
    out = []
    for name in sorted(kds):
        value, size = funcs[name]
        out.append((name, size, hashlib.sha256(text[value - base:value - base + size]).hexdigest()[:16]))
    return out


def units(objdir=OBJ):
    """(unit name, code object path, scratch directory) of every object with device code; the directory lives as long as
    the iteration step."""
    for f in sorted(os.listdir(objdir)):
        if not f.endswith('.o'):
            continue
        with tempfile.TemporaryDirectory() as td:
            co = unbundle(os.path.join(objdir, f), td)
            if co:
                yield f[:-2], co, td


def kernel_names(objdir=OBJ):
    """['unit mangled-kernel-name'], sorted: the set of kernels the build holds, per unit."""
    return ['%s %s' % (u, k[0]) for u, co, td in units(objdir) for k in kernels_of(co, td)]


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    objdir = args[0] if args else OBJ
    if '--names' in sys.argv:
        print('\n'.join(kernel_names(objdir)))
    elif '--kernels' in sys.argv:
        for u, co, td in units(objdir):
            for name, size, h in kernels_of(co, td):
                print(u, size, h, name)
    else:
        for u, co, td in units(objdir):
            text = text_of(co, td)
            print(u + '.o', hashlib.sha256(text).hexdigest()[:16] if text is not None else 'no text')
