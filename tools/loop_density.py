#!/usr/bin/env python3
"""Instruction mix of the MFMA loop of every kernel in one gfx950 code object.

    python tools/loop_density.py conv_gemm_patch.s [--match p8_kernel] [--json]
    hipcc --offload-arch=gfx950 -O3 ... -S --cuda-device-only -o x.s x.hip      # how to get the .s (Makefile flags)

Input: the device assembly of ONE source file (`-S --cuda-device-only`, or the `*-gfx950.s` of --save-temps), or an object file (a device ELF, or a host .o with the
bundled device code: it is unbundled and disassembled with llvm-objdump --symbolize-operands).  Per kernel symbol the tool finds the loops (a branch to a label
defined earlier), takes the INNERMOST loop that holds MFMAs (the one with the most MFMAs when there are several: the steady-state copy of a peeled loop -- the peeled
copies sit outside any inner loop) and prints
    mfma      number of MFMA instructions in the body
    other     every other instruction, by class: salu valu ds vmem (global / buffer / scratch, LDS-DMA included) waitcnt nop branch barrier
    gaps      the number of other instructions between consecutive MFMAs in program order, and `wrap`: from the last MFMA over the back edge to the first
A static count: both sides of a branch inside the body are counted (the two waves of a SIMD of conv_gemm_p8_kernel execute one copy each of every issue site).
MFMA-busy of this project's kernels follows `other / mfma`; tests/test_loop_density_cpu.py compares two instantiations of one compile with it."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN') or '/opt/rocm/llvm/bin'
CLASSES = ('salu', 'valu', 'ds', 'vmem', 'waitcnt', 'nop', 'branch', 'barrier')


def classify(mn):
    if mn.startswith(('v_mfma', 'v_smfmac')):
        return 'mfma'
    if mn.startswith('s_waitcnt'):
        return 'waitcnt'
    if mn in ('s_nop', 's_sleep'):
        return 'nop'
    if mn.startswith('s_barrier'):
        return 'barrier'
    if mn.startswith(('s_branch', 's_cbranch', 's_setpc', 's_swappc', 's_call', 's_endpgm')):
        return 'branch'
    if mn.startswith('s_'):
        return 'salu'
    if mn.startswith('ds_'):
        return 'ds'
    if mn.startswith(('global_', 'buffer_', 'flat_', 'scratch_', 'tbuffer_')):
        return 'vmem'
    return 'valu'


def _asm_text(path):
    """The assembly text of `path`; objects are disassembled."""
    with open(path, 'rb') as f:
        head = f.read(64)
    if not head.startswith((b'\x7fELF', b'__CLANG_OFFLOAD_BUNDLE__')):
        return open(path).read(), False
    with tempfile.TemporaryDirectory() as tmp:
        obj = path
        if head.startswith(b'\x7fELF') and head[18:20] != b'\xe0\x00':             # a host object (e_machine != EM_AMDGPU): its device code is a bundle in .hip_fatbin
            fat = os.path.join(tmp, 'fat.bin')
            subprocess.run([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', path, fat], check=True)
            obj = fat
            head = open(fat, 'rb').read(24)
        if head.startswith(b'__CLANG_OFFLOAD_BUNDLE__'):
            out = os.path.join(tmp, 'dev.o')
            subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + obj, '--output=' + out],
                           check=True)
            obj = out
        r = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--symbolize-operands', '--no-show-raw-insn', '--no-leading-addr', obj], check=True, capture_output=True,
                           text=True)
        return r.stdout, True


def kernels(path):
    """{symbol: [('label', name) | ('ins', mnemonic, operands)]} of every function in the file."""
    text, dis = _asm_text(path)
    out, cur = {}, None
    for line in text.splitlines():
        if dis:
            m = re.match(r'^[0-9a-f]* ?<([^>]+)>:\s*$', line)
            if m:
                if m.group(1).startswith('L') and m.group(1)[1:].isdigit() and cur is not None:
                    cur.append(('label', m.group(1)))
                else:
                    cur = out.setdefault(m.group(1), [])
                continue
            m = re.match(r'^<(L\d+)>:\s*$', line)
            if m and cur is not None:
                cur.append(('label', m.group(1)))
                continue
        else:
            m = re.match(r'^([A-Za-z_.$][\w.$]*):', line)
            if m:
                name = m.group(1)
                if name.startswith('.L'):
                    if name.startswith('.Lfunc_end'):
                        cur = None
                    elif cur is not None:
                        cur.append(('label', name))
                else:
                    cur = out.setdefault(name, [])
                continue
        if cur is None:
            continue
        body = line.split('//')[0].split(';')[0].strip()
        if not body or body.startswith('.'):
            continue
        parts = body.split(None, 1)
        if re.match(r'^[a-z][a-z0-9_]*$', parts[0]):
            cur.append(('ins', parts[0], parts[1] if len(parts) > 1 else ''))
    return {k: v for k, v in out.items() if any(e[0] == 'ins' for e in v)}


def mfma_loop(items):
    """The body (list of mnemonics) of the innermost loop with the most MFMAs, or None."""
    pos = {e[1]: i for i, e in enumerate(items) if e[0] == 'label'}
    loops = []
    for i, e in enumerate(items):
        if e[0] == 'ins' and classify(e[1]) == 'branch':
            m = re.search(r'(\.LBB\w+|\bL\d+\b)', e[2])
            if m and m.group(1) in pos and pos[m.group(1)] < i:
                loops.append((pos[m.group(1)], i))
    best = None
    for lo, hi in loops:
        n = sum(1 for e in items[lo:hi + 1] if e[0] == 'ins' and classify(e[1]) == 'mfma')
        if n == 0:
            continue
        if any((l2, h2) != (lo, hi) and lo <= l2 and h2 <= hi and any(e[0] == 'ins' and classify(e[1]) == 'mfma' for e in items[l2:h2 + 1]) for l2, h2 in loops):
            continue                                                    # an outer loop
        if best is None or n > best[0]:
            best = (n, lo, hi)
    if best is None:
        return None
    return [e[1] for e in items[best[1]:best[2] + 1] if e[0] == 'ins']


def density(body):
    cls = [classify(m) for m in body]
    at = [i for i, c in enumerate(cls) if c == 'mfma']
    gaps = [b - a - 1 for a, b in zip(at, at[1:])]
    wrap = at[0] + len(cls) - 1 - at[-1]
    by = {c: cls.count(c) for c in CLASSES}
    return {'mfma': len(at), 'other': len(cls) - len(at), 'by_class': by, 'gaps': gaps, 'wrap': wrap, 'max_gap': max(gaps + [wrap]),
            'other_per_mfma': round((len(cls) - len(at)) / len(at), 2)}


def metadata(path):
    """{symbol: {'vgpr_spill_count', 'private_segment_fixed_size', 'vgpr_count', 'sgpr_spill_count'}} from the amdhsa.kernels notes of an assembly file."""
    out, cur = {}, None
    for line in open(path, errors='replace'):
        m = re.match(r'\s+\.name:\s+(\S+)', line)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.match(r'\s+\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count|agpr_count):\s+(\d+)', line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
        if re.match(r'\s+-\s+\.a', line) or line.startswith('amdhsa.target'):
            pass
    return out


def demangle(names):
    try:
        r = subprocess.run([os.path.join(LLVM, 'llvm-cxxfilt')], input='\n'.join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def report(path, match=None):
    ks = kernels(path)
    res = {}
    for sym, items in ks.items():
        if match and match not in sym:
            continue
        body = mfma_loop(items)
        if body:
            res[sym] = density(body)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('file')
    ap.add_argument('--match', help='only symbols that contain this text (mangled name)')
    ap.add_argument('--json', action='store_true')
    a = ap.parse_args()
    res = report(a.file, a.match)
    if a.json:
        print(json.dumps(res))
        return 0
    nice = demangle(list(res))
    for sym, d in res.items():
        print(nice[sym])
        print('  mfma %d   other %d (%.2f per MFMA): %s' % (d['mfma'], d['other'], d['other_per_mfma'], '  '.join('%s %d' % (c, d['by_class'][c]) for c in CLASSES)))
        print('  gaps %s  wrap %d  (largest %d)' % (d['gaps'], d['wrap'], d['max_gap']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
