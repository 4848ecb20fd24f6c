#!/usr/bin/env python3
"""Is the gfx950 device code of two builds of one source file the same?  Disassembles both objects the way tools/loop_density.py does and compares every device
function instruction by instruction (mnemonics, operands and branch labels).  A host-only refactor must print `identical` for every object it touched.

    python tools/device_code_diff.py parent/conv_wgrad.o segland_amd/csrc/conv_wgrad.o
    python tools/device_code_diff.py parent/segland_amd/csrc segland_amd/csrc        # every *.o of two build directories; exit status 1 if any differs or is missing
    python tools/device_code_diff.py --added-ok parent/loss.o segland_amd/csrc/loss.o # a change that adds kernels: functions of the second object alone are listed, not counted

An instantiation whose template gained an argument has a new symbol; it is paired with the old one where the qualified name and every instruction are the same."""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_density  # noqa: E402

ADDED_OK = False


def local_labels(items):
    """Branch labels renumbered per function in order of appearance: the assembler numbers them through the whole object, so a function added in front of an untouched
    one would otherwise make it 'differ'."""
    seen = {}
    sub = lambda m: seen.setdefault(m.group(0), 'L#%d' % len(seen))
    return [tuple(re.sub(r'\bL\d+\b', sub, x) if isinstance(x, str) else x for x in it) for it in items]


def base_name(sym):
    """The qualified name of a mangled function without its template arguments and parameters (`_ZN12_GLOBAL__N_14nameILi16E...` -> `_GLOBAL__N_1::name`); the symbol
    itself where it is not of that shape."""
    m = re.match(r'_ZN?', sym)
    if not m:
        return sym
    at, parts = m.end(), []
    while True:
        d = re.match(r'\d+', sym[at:])
        if not d:
            break
        n = int(d.group(0))
        parts.append(sym[at + d.end():at + d.end() + n])
        at += d.end() + n
    return '::'.join(parts) or sym


def pair_renamed(a, b):
    """[(symbol of a, symbol of b)]: functions on one side only whose template gained or lost an argument -- the same qualified name and the same instructions.  A kernel
    template that takes one more parameter has new symbols for the instantiations it had; this is how `identical` is still shown for them."""
    only_a, only_b = [s for s in sorted(a) if s not in b], [s for s in sorted(b) if s not in a]
    pairs = []
    for sa in only_a:
        for sb in only_b:
            if base_name(sa) == base_name(sb) and a[sa] == b[sb]:
                pairs.append((sa, sb))
                only_b.remove(sb)
                break
    return pairs


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
    renamed = pair_renamed(a, b)
    for sa, sb in renamed:
        print('same code, new symbol: %s -> %s' % (nice[sa], nice[sb]))
    paired = {s for p in renamed for s in p}
    for sym in sorted(set(a) | set(b)):
        if sym in paired:
            continue
        if sym not in a or sym not in b:
            print('only in %s: %s' % (pa if sym in a else pb, nice[sym]))
            bad += sym in a or not ADDED_OK
        elif a[sym] != b[sym]:
            at = next((i for i, (x, y) in enumerate(zip(a[sym], b[sym])) if x != y), min(len(a[sym]), len(b[sym])))
            print('differs: %s (%d vs %d items, first at %d)' % (nice[sym], len(a[sym]), len(b[sym]), at))
            bad += 1
    print('%s: %d device functions, %d instructions, %s' % (os.path.basename(pb), len(b), sum(1 for v in b.values() for e in v if e[0] == 'ins'),
                                                           'identical' if not bad else '%d DIFFER' % bad))
    return bad


def main():
    global ADDED_OK
    args = [x for x in sys.argv[1:] if x != '--added-ok']
    ADDED_OK = len(args) != len(sys.argv) - 1
    pa, pb = args[:2]
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
