#!/usr/bin/env python
"""Static census of the Stage-II chain kernel's frame loop (CPU only: compiles to gfx950 assembly, runs nothing).

    python tools/loop_census.py [--source FILE] [--label TEXT] [--keep-asm FILE]

Compiles chain_solve.hip (or FILE, another version of it: the headers are taken from moshpp_amd/csrc) for the 4-block size class
(-DMOSHII_DEV_ONLY_NBLK4) with the flags of moshpp_amd/build.py and counts, for the one-workgroup and the cooperative kernel,
the instructions that only move values between register files and their arithmetic-free homes:

    v_readlane / v_writelane   scalars parked in the lanes of a vector register (SGPR spills)
    v_accvgpr_*                vector values parked in the accumulator half of the register file
    scratch_load / _store      ... and those that did not fit there either
    v_readfirstlane, s_nop, barriers

in three regions: the whole kernel body, the dogleg iteration loop (the loop of depth 3 that holds the calls of the forward
evaluation, the rigid init, the assembly and the solve: run_phase's `while (true)`) and the rest of the frame loop around it
(the loop of depth 1 that holds it, without it: frame head, phase set-up, record).  The regions come from the loop annotations
the compiler writes into the assembly.  Below the table: the compiler's own resource usage lines for the two kernels.

The counts move with the compiler; profiles/dogleg_loop_census.txt keeps one run for the record.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moshpp_amd import build as mbuild  # noqa: E402

KERNELS = (('one workgroup', '_ZN6moshii13k_chain_solveILi4ELi1ELb0ELb0EEE'), ('cooperative', '_ZN6moshii13k_chain_solveILi4ELi1ELb0ELb1EEE'))
KINDS = (('instructions', None),
         ('v_readlane', re.compile(r'^v_readlane_')),
         ('v_writelane', re.compile(r'^v_writelane_')),
         ('v_accvgpr_*', re.compile(r'^v_accvgpr_')),
         ('scratch_load', re.compile(r'^scratch_load_')),
         ('scratch_store', re.compile(r'^scratch_store_')),
         ('v_readfirstlane', re.compile(r'^v_readfirstlane_')),
         ('s_nop', re.compile(r'^s_nop$')),
         ('barriers', re.compile(r'^s_barrier')))
CALL = re.compile(r'^s_swappc_b64$')
LABEL = re.compile(r'^\.LBB(\d+_\d+):')
PARENT = re.compile(r'Parent Loop BB(\d+_\d+) Depth=(\d+)')
HEADER = re.compile(r'This (?:Inner )?Loop Header: Depth=(\d+)')
INLOOP = re.compile(r'in Loop: Header=BB(\d+_\d+) Depth=(\d+)')


def compile_asm(source, keep=None):
    """(assembly text, compiler remarks) of the 4-block development build of `source`."""
    out = keep or tempfile.NamedTemporaryFile(suffix='.s', delete=False).name
    cmd = ([mbuild._hipcc()] + mbuild.compile_flags('chain_solve.hip', defines=['-DMOSHII_DEV_ONLY_NBLK4'])
           + ['-I', mbuild.CSRC, '-S', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-x', 'hip', source, '-o', out])
    res = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stderr)
        raise SystemExit('hipcc failed')
    with open(out) as fh:
        text = fh.read()
    if not keep:
        os.unlink(out)
    return text, res.stderr


def kernel_lines(asm, mangled_prefix):
    lines = asm.split('\n')
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ':' in ln)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    return lines[start + 1:end]


def blocks_of(lines):
    """[(label or None, loop chain (outermost first) as [(header label, depth)], [mnemonic, ...])] in program order."""
    blocks = [[None, [], []]]
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = LABEL.match(ln)
        if m:
            note = ln
            j = i + 1
            while j < len(lines) and lines[j].lstrip().startswith(';'):
                note += '\n' + lines[j]
                j += 1
            chain = [(p, int(d)) for p, d in PARENT.findall(note)]
            h = HEADER.search(note)
            il = INLOOP.search(note)
            if h:
                chain.append((m.group(1), int(h.group(1))))
            elif il:
                chain = [('?' + il.group(1), int(il.group(2)))]   # resolved below: the chain of that header
            blocks.append([m.group(1), chain, []])
            i = j
            continue
        s = ln.strip()
        if ln.startswith('\t') and s and s[0] not in '.;':
            blocks[-1][2].append(s.split()[0])
        i += 1
    chains = {b[0]: b[1] for b in blocks if b[1] and not b[1][0][0].startswith('?')}
    for b in blocks:
        if b[1] and b[1][0][0].startswith('?'):
            b[1] = chains[b[1][0][0][1:]]
    return blocks


def count(mnemonics):
    return [len(mnemonics) if rx is None else sum(1 for m in mnemonics if rx.match(m)) for _, rx in KINDS]


def census(lines):
    blocks = blocks_of(lines)
    calls_in = {}
    for _, chain, mn in blocks:
        c = sum(1 for m in mn if CALL.match(m))
        for hd in chain:
            calls_in[hd] = calls_in.get(hd, 0) + c
    depth3 = [hd for hd in calls_in if hd[1] == 3]
    if not depth3:
        raise SystemExit('no loop of depth 3 in the kernel: the frame loop has changed shape')
    it = max(depth3, key=lambda hd: calls_in[hd])
    frame = next(chain[0] for _, chain, _ in blocks if it in chain)
    body = [m for _, _, mn in blocks for m in mn]
    loop = [m for _, chain, mn in blocks if it in chain for m in mn]
    rest = [m for _, chain, mn in blocks if frame in chain and it not in chain for m in mn]
    return (('whole kernel body', count(body)),
            ('dogleg iteration loop (BB%s, %d calls)' % (it[0], calls_in[it]), count(loop)),
            ('frame loop outside it (BB%s)' % frame[0], count(rest)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--source', default=os.path.join(mbuild.CSRC, 'chain_solve.hip'))
    ap.add_argument('--label', default='')
    ap.add_argument('--keep-asm', default=None)
    a = ap.parse_args()
    asm, remarks = compile_asm(a.source, a.keep_asm)
    print('== %s' % (a.label or os.path.relpath(a.source, ROOT)))
    for name, prefix in KERNELS:
        print('%s kernel, k_chain_solve<4, 1, false, %s>' % (name, 'true' if name == 'cooperative' else 'false'))
        rows = census(kernel_lines(asm, prefix))
        print('  %-44s' % 'region' + ''.join('%16s' % k for k, _ in KINDS))
        for region, c in rows:
            print('  %-44s' % region + ''.join('%16d' % v for v in c))
            moved = c[1] + c[2] + c[3] + c[4] + c[5]
            print('  %-44s%16d' % ('    lane + accumulator + scratch moves', moved))
        want = False
        for ln in remarks.split('\n'):
            if 'Function Name:' in ln:
                want = prefix in ln
            if want and 'remark:' in ln:
                print('  ' + ln.split('remark:', 1)[1].replace('[-Rpass-analysis=kernel-resource-usage]', '').rstrip())
        print()


if __name__ == '__main__':
    main()
