"""Static instruction density of conv_gemm_p8_kernel's K-tile body (tools/loop_density.py): the 1x1 form (K1 = true) against the generic form of the
same EPI, both from ONE compile of conv_gemm_patch.hip with the Makefile's flags -- the new code is compared with the kernel it replaces, not with a recorded number.
No GPU needed: hipcc cross-compiles for gfx950."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'segland_amd', 'csrc')
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _makefile_var(name, text):
    m = re.search(r'^%s\s*\??=\s*(.*)$' % name, text, re.M)
    return m.group(1).strip()


@pytest.fixture(scope='module')
def patch_asm(tmp_path_factory):
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    hipcc = os.environ.get('HIPCC') or _makefile_var('HIPCC', mk)
    flags = _makefile_var('CXXFLAGS', mk).replace('$(ARCH)', _makefile_var('ARCH', mk)).split()
    out = str(tmp_path_factory.mktemp('density') / 'conv_gemm_patch.s')
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', '-o', out, os.path.join(CSRC, 'conv_gemm_patch.hip')], check=True, capture_output=True)
    return out


def _sym(epi, k1, names):
    hit = [n for n in names if 'conv_gemm_p8_kernelILi%dELb%dEEE' % (epi, k1) in n]
    assert len(hit) == 1, (epi, k1, hit)
    return hit[0]


def test_loop_density_tool_finds_the_k_tile_bodies(patch_asm):
    import loop_density as ld
    rep = ld.report(patch_asm, 'conv_gemm_p8_kernel')
    assert len(rep) == 6, sorted(rep)
    for sym, d in rep.items():
        assert d['mfma'] == 32 and len(d['gaps']) == 31, (sym, d)                    # one K-tile: 4 phases x 4 k-steps x 2 MFMAs, peeled copies not counted
        assert d['other'] == sum(d['by_class'].values()) == sum(d['gaps']) + d['wrap'], (sym, d)
        assert d['by_class']['barrier'] == 2 and d['by_class']['ds'] == 24, (sym, d)  # two barriers and 24 fragment reads per K-tile (conv_gemm_patch.hip)


@pytest.mark.parametrize('epi', [0, 1, 2])
def test_p8_k1_body_is_at_most_half_of_the_generic_body(patch_asm, epi):
    """Other-than-MFMA instructions of the steady-state K-tile body: K1 at most half of the generic form, its largest gap between two MFMAs (the back edge included) at
    most 0.6 x; no K1 instantiation spills more VGPRs or uses more scratch than the generic one of the same EPI, and <0, K1> uses none."""
    import loop_density as ld
    rep = ld.report(patch_asm, 'conv_gemm_p8_kernel')
    meta = ld.metadata(patch_asm)
    gen, k1 = _sym(epi, 0, rep), _sym(epi, 1, rep)
    print('EPI %d generic: other %d gaps %s wrap %d | K1: other %d gaps %s wrap %d' % (epi, rep[gen]['other'], rep[gen]['gaps'], rep[gen]['wrap'], rep[k1]['other'], rep[k1]['gaps'],
                                                                                    rep[k1]['wrap']))
    print('EPI %d spilled VGPRs / scratch bytes: generic %d / %d, K1 %d / %d' % (epi, meta[gen]['vgpr_spill_count'], meta[gen]['private_segment_fixed_size'],
                                                                                meta[k1]['vgpr_spill_count'], meta[k1]['private_segment_fixed_size']))
    assert 2 * rep[k1]['other'] <= rep[gen]['other'], (rep[k1]['other'], rep[gen]['other'])
    assert rep[k1]['max_gap'] <= 0.6 * rep[gen]['max_gap'], (rep[k1]['max_gap'], rep[gen]['max_gap'])
    assert meta[k1]['vgpr_spill_count'] <= meta[gen]['vgpr_spill_count'] and meta[k1]['private_segment_fixed_size'] <= meta[gen]['private_segment_fixed_size'], (meta[k1], meta[gen])
    if epi == 0:
        assert meta[k1]['vgpr_spill_count'] == 0 and meta[k1]['private_segment_fixed_size'] == 0, meta[k1]
