"""CPU-only half of the exact-integer convolution tests (tests/conv_exact_cases.py; the launches are in test_conv_exact_gpu.py): host queries and the float64 reference.
Every table entry is on the kernel it names, every code the two dispatch chains can return has an entry, and the operand generator keeps the bounds that make the
comparison exact."""
import os

import pytest

import conv_exact_cases as cx
from segland_amd import _lib


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_every_table_entry_is_on_the_kernel_it_names(lib):
    """sl_conv2d_tile_config_ex(desc, mode, epi) / sl_conv2d_wgrad_config(desc) answer each entry's code, debug record at its defaults except the entry's own hooks."""
    wrong = [(cx.case_id(c), cx.query(lib, c)) for c in cx.TABLE if cx.query(lib, c) != c.code]
    assert not wrong, wrong
    for c in cx.TABLE:
        assert c.mode == cx.ENTRIES[c.entry][0] and c.epi == cx.ENTRIES[c.entry][1]


def test_fused_data_gradient_entries_are_served(lib):
    """The fused forms of the pixel-stationary kernel and the gated statistics have served-queries of their own: the table's entries are served shapes (an unserved one
    would make the wrapper return None and the GPU case fail)."""
    import ctypes as C
    for c in cx.TABLE:
        r = C.byref(cx.desc(c))
        if c.entry == 'bwd_bnstat':
            assert lib.sl_conv2d_bwd_data_bnstat_rows(r) > 0, cx.case_id(c)
        if c.entry in ('bwd_addend_bnstat', 'bwd_addend_bnstat2', 'bwd_addend_half_stats'):
            assert lib.sl_conv2d_bwd_data_addend_bnstat_rows(r) == c.B * c.H * c.W // 256, cx.case_id(c)
        if c.entry in ('bwd_addend_half', 'bwd_addend_half_stats'):
            assert lib.sl_conv2d_bwd_data_addend_half_ok(r) == 1, cx.case_id(c)
        if c.entry == 'affine_splitk':
            assert lib.sl_conv2d_affine_fwd_workspace(r) == 4 * c.B * c.H * c.W * c.cout * 4, cx.case_id(c)      # four parts of fp32 partial tiles


def test_every_code_of_the_forward_chain_has_an_exact_case():
    """The literals choose_kernel returns, read from csrc/conv_gemm.hip: each has a bf16 entry, the ones an fp32 launch can reach (also read from the source) an fp32
    entry.  A route added to the chain fails here until it has an exact case.  Asserted besides: a launch with the debug record at its defaults, a forward launch, a
    data-gradient launch, a ragged edge and a case of the wide operand set per code -- the exceptions are named with the predicate that rules them out."""
    codes, fp32 = cx.chain_codes(), cx.fp32_codes()
    assert len(codes) >= 15 and len(fp32) >= 6 and set(fp32) < set(codes)
    conv = [c for c in cx.TABLE if c.mode < 2]
    have = {(c.code, c.dtype) for c in conv}
    assert not [k for k in codes if (k, cx.BF) not in have], [k for k in codes if (k, cx.BF) not in have]
    assert not [k for k in fp32 if (k, cx.F32) not in have], [k for k in fp32 if (k, cx.F32) not in have]
    assert not [k for k, _ in have if k not in codes], 'the table names a code the chain no longer returns'
    assert set(codes) == {c.code for c in conv if not c.hooks}
    # forward: bf16 launches of big N % 256 layers go to the half-tile kernel first, so 4256256 has forward cases in fp32 only
    assert {c.code for c in conv if c.mode == 0 and c.dtype == cx.BF} == set(codes) - {4256256}
    assert {c.code for c in conv if c.mode == 0 and c.dtype == cx.F32} == set(fp32)
    # data gradient: split-K is planned for forward launches only (splitk_parts)
    assert {c.code for c in conv if c.mode == 1} == set(codes) - {18256256}
    assert {c.code for c in conv if c.mode == 1 and c.dtype == cx.F32} >= {2128128, 4128128}
    # the second operand set reaches the plain store of every code; 18256256 has none (split-K serves the affine forms only, whose epilogue works on the accumulator
    # already rounded to the tensor type: past 256 that is two roundings by design)
    assert {c.code for c in conv if c.wide} == set(codes) - {18256256}
    assert all(c.entry in ('fwd', 'fwd_stats', 'bwd') for c in conv if c.wide)
    # ragged edges (a last row block that is not full; 16 x 16 tiles that overhang the map).  Not admitted: 8256256 / 18256256 (p9_shape: H, W multiples of 16),
    # 6256064 (sk_shape: M % 256 == 0) and the parity planes (parity_shape: hw % 256 == 0)
    def ragged(c):
        if c.code in cx.TILE16:
            return bool(c.H % 16 or c.W % 16)
        return (c.B * c.H * c.W) % ((c.code // 1000) % 1000) != 0
    assert {c.code for c in conv if ragged(c) and c.dtype == cx.BF} == set(codes) - {8256256, 18256256, 6256064}
    assert {c.code for c in conv if ragged(c) and c.dtype == cx.F32} >= {2128064, 2128128, 4128128, 2256064, 4256128, 4256256}
    assert not [cx.case_id(c) for c in conv if ragged(c) and cx.is_parity(c)]


def test_every_answer_of_the_weight_gradient_plan_has_an_exact_case():
    """enum WgradRoute's special routes 1, 2, 3 and, for the tile route, every (BNN, BCC) the launch switch of csrc/conv_wgrad.hip instantiates and plan() can emit,
    the pixel-pair form and fp32; and for each answer every call form plan_wgrad admits on it.  ((128, 128) of the register-staged kernel is instantiated but not planned:
    both sides at 128-multiples is the glds kernel's rule.)"""
    routes, glds, staged = cx.wgrad_codes()
    wg = [c for c in cx.TABLE if c.mode == 2]
    tiles = [10000000 + 1000 * a + b for a, b in glds] + [20000000 + 1000 * a + b for a, b in staged if (a, b) != (128, 128)]
    pairs = {c.code for c in wg if c.code // 500000 % 2 == 1}
    assert routes == [1, 2, 3] and pairs, 'a new special route, or no pixel-pair case'

    def forms(code, dtype=cx.BF):
        """(entry, second source?, sl_debug_wgrad_bias(0)?) of the cases with this answer"""
        return {(c.entry, bool(c.c1), ('sl_debug_wgrad_bias', 0) in c.hooks) for c in wg if c.code == code and c.dtype == dtype}
    plain = {(e, False, False) for e in ('wgrad', 'wgrad_off', 'wgrad_clip', 'wgrad_bias')}
    x2, kb = ('wgrad', True, False), ('wgrad_bias', False, True)
    # route 1: one source, own dw, unclipped (c64k3_eligible, `full`); route 2: one source (c64p_eligible); route 3: unclipped (`full`).  Their bias rows are the
    # stand-alone pass whatever the hook says.
    assert forms(1) == {('wgrad', False, False), ('wgrad_bias', False, False)}
    assert forms(2) == plain
    assert forms(3) == {('wgrad', False, False), ('wgrad_off', False, False), ('wgrad_bias', False, False), x2}
    for code in tiles:
        want = set(plain)
        if code not in pairs:
            want.add(x2)                                    # pixel pairs need c2 == 0 (plan())
        if code // 10000000 == 1 and code % 500000 != 256256:
            want.add(kb)                                    # WB_KERNEL -> WB_REDUCE / WB_PASS; 256 x 256 and the register-staged kernel never take the bias partials
        assert forms(code) >= want, (code, sorted(want - forms(code)))
    for code in pairs:
        assert forms(code) >= plain | {kb}, code
    assert forms(10128128, cx.F32) >= plain | {x2, kb} and forms(20064064, cx.F32) >= plain | {x2}
    assert any(('sl_debug_wgrad_tr', 0) in c.hooks for c in wg if c.code // 10000000 == 1) and any(('sl_debug_wgrad_tr', 0) in c.hooks for c in wg if c.code // 10000000 == 2)
    # a case that names a hook-only plan says so: the query (test_every_table_entry_is_on_the_kernel_it_names) and the launch both run with exactly the case's hooks
    assert [c.hooks for c in wg if c.entry == 'wgrad_clip' and c.k == 3 and c.code == 10128128] == [(('sl_debug_wgrad3', 0),)]


SMALL = [c for c in cx.TABLE if c.B * c.H * c.W * c.cin * c.cout * c.k * c.k <= 2048 * 64 * 128 * 9 or c.code == 18256256]


@pytest.mark.parametrize('c', SMALL, ids=[cx.case_id(c) for c in SMALL])
def test_reference_keeps_the_bounds_that_make_it_exact(c):
    """The cases whose float64 reference takes well under a second: integral values (multiples of 0.25 behind an affine epilogue), magnitudes and statistics partials
    below 2^24, at most 256 wherever the kernel consumes its output again -- asserted on the reference alone (cx.check_bounds), as the GPU test does for every case."""
    e = cx.expected(c)
    cx.check_bounds(c, e)
    assert cx.to_dtype(e['out'], c.dtype).dtype == c.dtype
