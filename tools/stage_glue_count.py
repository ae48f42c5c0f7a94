#!/usr/bin/env python3
"""Static count of the stage machine's glue in a step kernel (fb_step.hpp: d_run), from the assembly hipcc emits (no GPU needed):
for every stage call of the kernel, the instructions that lie between the previous call and this one in the assembly -- scratch loads, scratch
stores, vector instructions, lane reads / writes of spilled scalar registers.  The interpreter's cases follow each other in the layout, so a
region is the glue in front of that call (dispatch included; the first region of a copy also holds the kernel's prologue or the ticket
loop's head): comparable between two builds, not a cycle count.  The interpreter is inlined twice in k_fly -- per-wave path first, ticket path
second; a copy starts at its s_pre call.
stage_glue_count.py [kernel substring, default _Z5k_flyIdE] [extra hipcc flags...]   or   stage_glue_count.py --asm FILE [kernel substring]"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
args = sys.argv[1:]
if args and args[0] == '--asm':
    path = args[1]; kern = args[2] if len(args) > 2 else '_Z5k_flyIdE'; lines = open(path).read().splitlines()
else:
    kern = args[0] if args and not args[0].startswith('-') else '_Z5k_flyIdE'
    flags = [a for a in args if a.startswith('-')]
    sys.path.insert(0, ROOT)
    from __graft_entry__ import hip_flags
    out = os.path.join(tempfile.gettempdir(), 'fb_engine_glue_%d.s' % os.getpid())
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--offload-arch=gfx950', '-O3', '-std=c++17', *hip_flags(), '--cuda-device-only', '-S',
                           '-o', out] + flags + [os.path.join(ROOT, 'flybody_amd', 'csrc', 'fb_engine.hip')], stderr=subprocess.DEVNULL)
    lines = open(out).read().splitlines(); os.unlink(out)
a = next(i for i, l in enumerate(lines) if re.match(r'^_Z\w*:', l) and kern in l)
b = next(i for i in range(a, len(lines)) if lines[i].startswith('.Lfunc_end'))
calls, tgt = [], '?'
for i in range(a, b):
    m = re.search(r'(_Z\w+)@rel32@lo', lines[i])
    if m: tgt = re.split(r'I[df]', re.sub(r'^_Z\d+', '', m.group(1)))[0]
    if 's_swappc' in lines[i]: calls.append((i, tgt))
PRE = ('scratch_load', 'scratch_store', 'v_', 'v_readlane', 'v_writelane', 'v_mov_b32')
def count(lo, hi):
    body = [x.strip() for x in lines[lo:hi] if x.startswith('\t') and not x.strip().startswith(('.', ';'))]
    return [sum(x.startswith(p) for x in body) for p in PRE] + [len(body)]
print('%-26s %6s %6s %6s %6s %6s %6s %6s' % ('region ending at call of', 'sc_ld', 'sc_st', 'vector', 'rdlane', 'wrlane', 'v_mov', 'all'))
prev, copy = a, 0
for i, t in calls:
    if t == 's_pre' and not (calls.index((i, t)) and calls[calls.index((i, t)) - 1][1] == 's_pre'):
        copy += 1; print('-- copy %d' % copy)
    print('%-26s %6d %6d %6d %6d %6d %6d %6d' % ((t,) + tuple(count(prev + 1, i + 1))))
    prev = i
print('%-26s %6d %6d %6d %6d %6d %6d %6d' % (('kernel',) + tuple(count(a, b))))
