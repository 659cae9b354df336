#!/usr/bin/env python3
"""Loop skeleton of one kernel's ISA: LDS and global reads / stores, every s_waitcnt, barriers, branches and labels in
program order, runs of MFMAs as counts, and the kernel's register / occupancy metadata.  (tools/isa_outline.py shows the
global side only.)
usage: hipcc -O3 --offload-arch=gfx950 -std=c++17 -S --cuda-device-only -o eng.s ga3c_amd/csrc/ga3c_engine.hip
       tools/isa_skeleton.py eng.s <mangled-name substring> [max lines]"""
import re
import sys

lines = open(sys.argv[1]).read().split('\n')
start = next(i for i, l in enumerate(lines) if l.startswith('_ZN') and sys.argv[2] in l.split(':')[0])
print(lines[start].split(':')[0])
out, run, end = [], [None, 0], start


def flush():
    if run[1]:
        out.append('    %s x%d' % (run[0], run[1]))
    run[0], run[1] = None, 0


for i, l in enumerate(lines[start + 1:], start + 1):
    if 's_endpgm' in l:
        end = i
        break
    t = l.strip().split(';')[0].strip()
    if not t:
        continue
    op = t.split()[0]
    if re.match(r'v_mfma|ds_read|ds_write|global_load|global_store|buffer_load', op):
        key = op + (' lds' if ' lds' in t else '')
        if run[0] != key:
            flush()
            run[0] = key
        run[1] += 1
    elif re.match(r's_waitcnt|s_barrier|s_cbranch|s_branch', op) or re.match(r'\.LBB\S+:', t):
        flush()
        out.append(('' if t.startswith('.LBB') else '    ') + t)
flush()
print('\n'.join(out[:int(sys.argv[3]) if len(sys.argv) > 3 else 400]))
for l in lines[end:]:
    if re.search(r'; (NumVgprs|NumAgprs|TotalNumVgprs|Occupancy|ScratchSize|LDSByteSize)', l):
        print(l.strip())
    if l.startswith('_ZN') or '.end_amdhsa_kernel' in l and 'Occupancy' in l:
        break
    if '; Occupancy' in l:
        break
