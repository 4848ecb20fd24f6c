"""Static instruction density of conv_gemm_p9_kernel's K-tile loop (tools/loop_density.py): every lean instantiation (D = 1 / 2 / 4, plain and flipped
window) against the generic loop (D = 0) of the same EPI, all from ONE compile of conv_gemm_patch.hip with the Makefile's flags -- the new code is compared with the
kernel it replaces, not with a recorded number.  The generic body is one K-tile (32 MFMAs), the lean body one chunk (nine K-tiles, 288 MFMAs), so the comparison is per
MFMA.  No GPU needed: hipcc cross-compiles for gfx950."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'segland_amd', 'csrc')
sys.path.insert(0, os.path.join(ROOT, 'tools'))

# EPI -> the lean instantiations launch_p9 uses: (D, FLIP).  Split-K (EPI 2) is planned for forward convs only.
LEAN = {0: [(d, f) for d in (1, 2, 4) for f in (0, 1)], 1: [(d, f) for d in (1, 2, 4) for f in (0, 1)], 2: [(d, 0) for d in (1, 2, 4)]}


def _makefile_var(name, text):
    m = re.search(r'^%s\s*\??=\s*(.*)$' % name, text, re.M)
    return m.group(1).strip()


@pytest.fixture(scope='module')
def patch_asm(tmp_path_factory):
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    hipcc = os.environ.get('HIPCC') or _makefile_var('HIPCC', mk)
    flags = _makefile_var('CXXFLAGS', mk).replace('$(ARCH)', _makefile_var('ARCH', mk)).split()
    out = str(tmp_path_factory.mktemp('density9') / 'conv_gemm_patch.s')
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', '-o', out, os.path.join(CSRC, 'conv_gemm_patch.hip')], check=True, capture_output=True)
    return out


def _sym(epi, d, flip, names):
    hit = [n for n in names if 'conv_gemm_p9_kernelILi%dELi%dELb%dEEE' % (epi, d, flip) in n]
    assert len(hit) == 1, (epi, d, flip, hit)
    return hit[0]


def test_loop_density_tool_finds_the_p9_bodies(patch_asm):
    import loop_density as ld
    rep = ld.report(patch_asm, 'conv_gemm_p9_kernel')
    assert len(rep) == 3 + sum(len(v) for v in LEAN.values()), sorted(rep)
    for epi in LEAN:
        g = rep[_sym(epi, 0, 0, rep)]
        assert g['mfma'] == 32 and g['by_class']['ds'] == 32, g                       # one K-tile: 24 fragment reads (4 B1, 8 A1, 4 B0, 8 A0) + the 8 A0 reads behind a single patch buffer's refill
        for d, f in LEAN[epi]:
            b = rep[_sym(epi, d, f, rep)]
            assert b['mfma'] == 288 and b['by_class']['ds'] == 8 * 27, (epi, d, f, b)  # one chunk: nine K-tiles, 24 fragment reads each
            assert b['other'] == sum(b['by_class'].values()) == sum(b['gaps']) + b['wrap'], (epi, d, f, b)


@pytest.mark.parametrize('epi', [0, 1, 2])
def test_p9_lean_body_is_at_most_a_quarter_of_the_generic_body_per_mfma(patch_asm, epi):
    """Other-than-MFMA instructions per MFMA of the steady-state body: every lean instantiation at most a quarter of the generic loop's (the lean forms reach 1.9 - 2.1
    per MFMA against 10.5: fragment reads and their waits are most of what is left, so a quarter is the structure's reach with a margin for compiler drift, a half would
    already pass with the per-read address arithmetic back in); the largest gap between two MFMAs (the back edge included) at most half of the generic loop's; no lean
    instantiation spills a VGPR or uses scratch."""
    import loop_density as ld
    rep = ld.report(patch_asm, 'conv_gemm_p9_kernel')
    meta = ld.metadata(patch_asm)
    gen = rep[_sym(epi, 0, 0, rep)]
    print('EPI %d generic: mfma %d other %d (%.2f per MFMA) %s largest gap %d' % (epi, gen['mfma'], gen['other'], gen['other'] / gen['mfma'], gen['by_class'], gen['max_gap']))
    for d, f in LEAN[epi]:
        sym = _sym(epi, d, f, rep)
        b, m = rep[sym], meta[sym]
        print('EPI %d lean d = %d flip %d: mfma %d other %d (%.2f per MFMA) %s largest gap %d wrap %d | VGPRs %d spilled %d scratch %d' % (
            epi, d, f, b['mfma'], b['other'], b['other'] / b['mfma'], b['by_class'], b['max_gap'], b['wrap'], m['vgpr_count'], m['vgpr_spill_count'], m['private_segment_fixed_size']))
        assert 4 * b['other'] * gen['mfma'] <= gen['other'] * b['mfma'], (d, f, b['other'], b['mfma'], gen['other'], gen['mfma'])
        assert 2 * b['max_gap'] <= gen['max_gap'], (d, f, b['max_gap'], gen['max_gap'])
        assert m['vgpr_spill_count'] == 0 and m['private_segment_fixed_size'] == 0, (d, f, m)
