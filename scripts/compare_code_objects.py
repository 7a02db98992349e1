#!/usr/bin/env python3
"""Are the device kernels of two builds the same machine code?
    python scripts/compare_code_objects.py DIR_A DIR_B          (each directory: the .o files of one build, e.g. two csrc/)
For every object: the .hip_fatbin section (llvm-objcopy --dump-section), its hipv4-amdgcn-amd-amdhsa--gfx950 entry
(clang-offload-bundler), the symbol table (llvm-readelf -s); per kernel the bytes of its FUNC symbol in .text and its 64-byte
descriptor NAME.kd in .rodata.  Kernels are matched by mangled name across the whole build, not per file, so code may move between
translation units.  Reported: names only in A, names only in B, kernels whose code bytes differ, kernels whose descriptor differs
with the entry-offset field (bytes 16-23: where the kernel sits in its code object) masked.  Exit status 0 only when all four
lists are empty.  Bytes and sizes only: nothing is disassembled.  Used on the build machine to hold a pure move of kernel sources
to "not one byte of any kernel changed" (profiles/csrc_split.md)."""
import os
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
KD_BYTES = 64
KD_ENTRY = slice(16, 24)            # kernel_code_entry_byte_offset: the distance from the descriptor to the code


def _run(tool, *args):
    r = subprocess.run([os.path.join(LLVM, tool)] + list(args), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('%s %s failed:\n%s' % (tool, ' '.join(args), r.stderr[-2000:]))
    return r.stdout


def _sections(co):
    """name -> (address, file offset, size, index) from `llvm-readelf -S`"""
    out = {}
    for line in _run('llvm-readelf', '-S', '-W', co).splitlines():
        if not line.lstrip().startswith('['):
            continue
        idx, rest = line.split(']', 1)
        f = rest.split()
        if len(f) < 5 or idx.strip(' [') == 'Nr':
            continue
        try:
            out[f[0]] = (int(f[2], 16), int(f[3], 16), int(f[4], 16), int(idx.strip(' [')))
        except ValueError:
            pass
    return out


def _symbols(co):
    """(name, value, size, type, section index) of every defined symbol from `llvm-readelf -s`: of .symtab, which holds the local
    symbols too (.dynsym, printed first, repeats the global ones)"""
    tables, cur = {}, None
    for line in _run('llvm-readelf', '-s', '-W', co).splitlines():
        if line.startswith('Symbol table '):
            cur = tables.setdefault(line.split("'")[1], [])
            continue
        f = line.split()
        if cur is None or len(f) != 8 or not f[0].endswith(':') or not f[0][:-1].isdigit() or not f[6].isdigit():
            continue
        cur.append((f[7], int(f[1], 16), int(f[2], 0), f[3], int(f[6])))
    return tables['.symtab'] if '.symtab' in tables else tables.get('.dynsym', [])


def code_object_kernels(co):
    """kernels of one gfx950 code object: [(mangled name, code bytes, descriptor bytes with the entry offset zeroed)]"""
    sec = _sections(co)
    by_index = {v[3]: v for v in sec.values()}
    blob = open(co, 'rb').read()
    syms = _symbols(co)

    def data(value, size, shndx):
        addr, off, ssize, _ = by_index[shndx]
        assert addr <= value and value + size <= addr + ssize, (co, value, size, shndx)
        return blob[off + value - addr: off + value - addr + size]

    funcs = {name: (value, size, shndx) for name, value, size, typ, shndx in syms if typ == 'FUNC'}
    out = []
    for name, value, size, typ, shndx in syms:
        if typ != 'OBJECT' or not name.endswith('.kd'):
            continue
        if size != KD_BYTES or shndx != sec['.rodata'][3]:
            raise RuntimeError('%s: descriptor %s is not %d bytes of .rodata' % (co, name, KD_BYTES))
        fv, fs, fx = funcs[name[:-3]]
        if fx != sec['.text'][3]:
            raise RuntimeError('%s: kernel %s is not in .text' % (co, name[:-3]))
        kd = bytearray(data(value, size, shndx))
        kd[KD_ENTRY] = bytes(8)
        out.append((name[:-3], data(fv, fs, fx), bytes(kd)))
    return out


def object_kernels(obj, tmp):
    """kernels of the gfx950 code object bundled in one host object (none: the object has no device code)"""
    fb, co = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'code_object')
    for p in (fb, co):
        if os.path.exists(p):
            os.remove(p)
    # (objcopy rewrites its input when no output is named)
    r = subprocess.run([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fb, obj, os.path.join(tmp, 'copy.o')],
                       capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(fb):
        return []
    _run('clang-offload-bundler', '--unbundle', '--type=o', '--targets=' + TARGET, '--input=' + fb, '--output=' + co)
    if not os.path.exists(co) or os.path.getsize(co) == 0:
        return []
    return code_object_kernels(co)


def build_kernels(directory):
    """mangled name -> sorted [(code, descriptor, object file)] over every .o of a build; a name can stand in several objects
    (an instantiation of a kernel template that a header holds)"""
    out = {}
    objs = sorted(f for f in os.listdir(directory) if f.endswith('.o'))
    if not objs:
        raise RuntimeError('no .o files in ' + directory)
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            for name, code, kd in object_kernels(os.path.join(directory, o), tmp):
                out.setdefault(name, []).append((code, kd, o))
    for v in out.values():
        v.sort()
    return out, objs


def compare(dir_a, dir_b):
    """the four lists: names only in A, names only in B, names whose code differs, names whose descriptor differs"""
    a, objs_a = build_kernels(dir_a)
    b, objs_b = build_kernels(dir_b)
    only_a = sorted(n for n in a if n not in b or len(a[n]) > len(b[n]))
    only_b = sorted(n for n in b if n not in a or len(b[n]) > len(a[n]))
    code, desc = [], []
    for n in sorted(set(a) & set(b)):
        if len(a[n]) != len(b[n]):
            continue
        if [x[0] for x in a[n]] != [x[0] for x in b[n]]:
            code.append((n, [(x[2], len(x[0])) for x in a[n]], [(x[2], len(x[0])) for x in b[n]]))
        if sorted(x[1] for x in a[n]) != sorted(x[1] for x in b[n]):
            desc.append((n, [x[2] for x in a[n]], [x[2] for x in b[n]]))
    counts = (len(objs_a), sum(len(v) for v in a.values()), len(objs_b), sum(len(v) for v in b.values()))
    return only_a, only_b, code, desc, counts


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    only_a, only_b, code, desc, counts = compare(sys.argv[1], sys.argv[2])
    print('A: %d objects, %d kernels; B: %d objects, %d kernels' % counts)
    print('only in A (%d):' % len(only_a))
    for n in only_a:
        print('  ' + n)
    print('only in B (%d):' % len(only_b))
    for n in only_b:
        print('  ' + n)
    print('code bytes differ (%d):' % len(code))
    for n, xa, xb in code:
        print('  %s   A %s   B %s' % (n, xa, xb))
    print('descriptor differs (%d):' % len(desc))
    for n, xa, xb in desc:
        print('  %s   A %s   B %s' % (n, xa, xb))
    same = not (only_a or only_b or code or desc)
    print('SAME' if same else 'DIFFERENT')
    sys.exit(0 if same else 1)


if __name__ == '__main__':
    main()
