#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of an engine library, function by function.

    python tools/kernel_isa_diff.py OLD.so NEW.so

Extracts the gfx950 code object of both shared objects (llvm-objcopy of .hip_fatbin, clang-offload-bundler), disassembles them
(llvm-objdump) and compares every kernel and device function by its instruction text.  Two things that move with the code AROUND a
function are left out of the comparison: the literal of the pc-relative address computation behind s_getpc_b64 (call targets, tables),
and the alignment padding behind a function's last instruction.  Prints the functions that differ, those only one build has, and
exits 1 if a function both builds have differs.  (the step kernels' code is held fixed while kernels are added.)
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')


def functions(so, workdir, tag, arch='gfx950'):
    fat, co = os.path.join(workdir, tag + '.fatbin'), os.path.join(workdir, tag + '.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', so, fat])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--' + arch,
                           '--input=' + fat, '--output=' + co, '--unbundle'])
    dis = subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--no-leading-addr', co], text=True)
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r'^[0-9a-f]* ?<(.+)>:$', line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith('Disassembly of section'):
            cur = None
        elif cur is not None and line.strip():
            cur.append(re.sub(r'\s*//.*$', '', line).strip())
    for ls in out.values():
        while ls and ls[-1].startswith(('s_nop', 's_code_end', '...')):
            ls.pop()
        for i, l in enumerate(ls):
            if l.startswith('s_getpc_b64'):
                for j in (i + 1, i + 2):
                    if j < len(ls) and re.match(r's_addc?_u32 ', ls[j]):
                        ls[j] = re.sub(r'(0x[0-9a-f]+|-?\d+)$', '<pcrel>', ls[j])
    return out


def main(old, new):
    with tempfile.TemporaryDirectory() as d:
        a, b = functions(old, d, 'old'), functions(new, d, 'new')
    diff = [n for n in a if n in b and a[n] != b[n]]
    print('%d functions in %s, %d in %s: %d identical, %d different' % (len(a), old, len(b), new, sum(n in b for n in a) - len(diff), len(diff)))
    for n in diff:
        k = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
        print('  DIFFERENT %s: %d / %d instructions, first difference at %d' % (n, len(a[n]), len(b[n]), k))
    for n in a:
        if n not in b:
            print('  only in old: %s (%d instructions)' % (n, len(a[n])))
    for n in b:
        if n not in a:
            print('  only in new: %s (%d instructions)' % (n, len(b[n])))
    return 1 if diff else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
