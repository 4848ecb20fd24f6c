#!/usr/bin/env python3
"""Is the gfx950 device code of two builds of one source file the same?  Disassembles both objects the way tools/loop_density.py does and compares every device
function instruction by instruction (mnemonics, operands and branch labels).  A host-only refactor must print `identical` for every object it touched.

    python tools/device_code_diff.py parent/conv_wgrad.o segland_amd/csrc/conv_wgrad.o
    python tools/device_code_diff.py parent/segland_amd/csrc segland_amd/csrc        # every *.o of two build directories; exit status 1 if any differs or is missing"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_density  # noqa: E402


def local_labels(items):
    """Branch labels renumbered per function in order of appearance: the assembler numbers them through the whole object, so a function added in front of an untouched
    one would otherwise make it 'differ'."""
    seen = {}
    sub = lambda m: seen.setdefault(m.group(0), 'L#%d' % len(seen))
    return [tuple(re.sub(r'\bL\d+\b', sub, x) if isinstance(x, str) else x for x in it) for it in items]


def diff_objects(pa, pb):
    """Prints what differs and one summary line for the pair; the number of device functions that differ or exist on one side only."""
    def functions(p):
        try:
            return {k: local_labels(v) for k, v in loop_density.kernels(p).items()}
        except subprocess.CalledProcessError:        # nothing to disassemble: a host-only object (api.o)
            return None
    a, b = functions(pa), functions(pb)
    if a is None or b is None:
        print('%s: %s' % (os.path.basename(pb), 'no device code on either side' if a is b else 'device code on one side only'))
        return 0 if a is b else 1
    nice = loop_density.demangle(sorted(set(a) | set(b)))
    bad = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            print('only in %s: %s' % (pa if sym in a else pb, nice[sym]))
            bad += 1
        elif a[sym] != b[sym]:
            at = next((i for i, (x, y) in enumerate(zip(a[sym], b[sym])) if x != y), min(len(a[sym]), len(b[sym])))
            print('differs: %s (%d vs %d items, first at %d)' % (nice[sym], len(a[sym]), len(b[sym]), at))
            bad += 1
    print('%s: %d device functions, %d instructions, %s' % (os.path.basename(pb), len(b), sum(1 for v in b.values() for e in v if e[0] == 'ins'),
                                                           'identical' if not bad else '%d DIFFER' % bad))
    return bad


def main():
    pa, pb = sys.argv[1:3]
    if not (os.path.isdir(pa) and os.path.isdir(pb)):
        return 1 if diff_objects(pa, pb) else 0
    # two build directories: every *.o that both hold, one line each; an object on one side only counts as a difference
    objs = [sorted(f for f in os.listdir(p) if f.endswith('.o')) for p in (pa, pb)]
    bad = 0
    for name in sorted(set(objs[0]) | set(objs[1])):
        if name not in objs[0] or name not in objs[1]:
            print('%s: only in %s' % (name, pa if name in objs[0] else pb))
            bad += 1
        else:
            bad += diff_objects(os.path.join(pa, name), os.path.join(pb, name))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
