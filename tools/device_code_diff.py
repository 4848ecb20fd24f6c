#!/usr/bin/env python3
"""Is the gfx950 device code of two builds of one source file the same?  Disassembles both objects the way tools/loop_density.py does and compares every device
function instruction by instruction (mnemonics, operands and branch labels).  A host-only refactor must print `identical` for every object it touched.

    python tools/device_code_diff.py parent/conv_wgrad.o segland_amd/csrc/conv_wgrad.o"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_density  # noqa: E402


def local_labels(items):
    """Branch labels renumbered per function in order of appearance: the assembler numbers them through the whole object, so a function added in front of an untouched
    one would otherwise make it 'differ'."""
    seen = {}
    sub = lambda m: seen.setdefault(m.group(0), 'L#%d' % len(seen))
    return [tuple(re.sub(r'\bL\d+\b', sub, x) if isinstance(x, str) else x for x in it) for it in items]


def main():
    a, b = ({k: local_labels(v) for k, v in loop_density.kernels(p).items()} for p in sys.argv[1:3])
    nice = loop_density.demangle(sorted(set(a) | set(b)))
    bad = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            print('only in %s: %s' % (sys.argv[1] if sym in a else sys.argv[2], nice[sym]))
            bad += 1
        elif a[sym] != b[sym]:
            at = next((i for i, (x, y) in enumerate(zip(a[sym], b[sym])) if x != y), min(len(a[sym]), len(b[sym])))
            print('differs: %s (%d vs %d items, first at %d)' % (nice[sym], len(a[sym]), len(b[sym]), at))
            bad += 1
    print('%s: %d device functions, %d instructions, %s' % (os.path.basename(sys.argv[2]), len(b), sum(1 for v in b.values() for e in v if e[0] == 'ins'),
                                                           'identical' if not bad else '%d DIFFER' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
