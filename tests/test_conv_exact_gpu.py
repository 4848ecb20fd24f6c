"""Every dispatch route of the implicit-GEMM convolutions against an exact integer reference, bit for bit (tests/conv_exact_cases.py holds the table, the operand
generator and the float64 reference; test_conv_exact_cpu.py proves the table covers both dispatch chains).

Each case asserts that the host query still answers the entry's kernel code (a threshold change cannot move the case to another kernel unnoticed), asserts the bounds
that make the comparison exact on the reference alone, runs the entry point through segland_amd.ops and compares with torch.equal: the output tensor in its type, the
statistic partials per partial row and in total, the weight gradient and the bias column sums.  No tolerance anywhere.

Partial rows: one per BM consecutive rows (BM from the code); for the patch kernels (7016016, 8256256) one per 16 x 16-pixel tile (b, y / 16, x / 16) -- their row blocks
ARE such tiles (ConvGemmParams::tile16).  The four launches of a parity-plane plan interleave their rows over the map; their partials are compared in total.

Not here: the GELU epilogues (SL_EPI_GELU, linear_fwd(want_gelu)) are not exact on integers and stay with their tolerance tests."""
import ctypes as C

import pytest
import torch

import conv_exact_cases as cx
from segland_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def g(t, dtype):
    return t.to(torch.float32).to(dtype).to(DEV).contiguous()


def gate_bits(ops, e, dtype):
    """The ReLU bits of the integer gate source, made by the product's own bn_act."""
    src = g(e['gate'], dtype)
    one = torch.ones(src.shape[-1], device=DEV)
    return ops.bn_act(src, one, torch.zeros_like(one), relu=True, want_mask=True)[1]


def check_partials(c, part, pairs, what):
    """part [rows][2][C] fp32 against the float64 per-element terms (a, b): totals, and each partial row."""
    for which, t in enumerate(pairs):
        tot = t.reshape(-1, t.shape[-1]).sum(0)
        assert torch.equal(part[:, which].double().sum(0).cpu(), tot), '%s: total of partial %d' % (what, which)
        blocks = cx.block_sums(t, c)
        if blocks is not None:
            assert part.shape[0] == blocks.shape[0], (what, part.shape, blocks.shape)
            assert torch.equal(part[:, which].double().cpu(), blocks), '%s: partial rows of %d' % (what, which)


def run_fwd(ops, c, p, e):
    spec = ops.ConvSpec(c.cin, c.cout, c.k, c.stride, c.pad, c.dil)
    wf, _ = ops.weight_prep(p.w.float().to(DEV), c.dtype, want_bwd=False)
    x = g(cx.nhwc(p.x), c.dtype)
    part = None
    if c.entry in ('fwd', 'fwd_stats'):
        y, part = ops.conv2d_fwd(x, wf, spec, want_stats=c.entry == 'fwd_stats')
    else:
        res, pre = (g(e['res'], c.dtype), g(e['pre'], c.dtype)) if c.entry == 'affine_res' else (None, None)
        y = ops.conv2d_affine_fwd(x, wf, spec, g(e['scale'], torch.float32), g(e['shift'], torch.float32), residual=res, relu=True, pre_addend=pre)
    assert torch.equal(y.cpu(), cx.to_dtype(e['out'], c.dtype)), 'output'
    if 'stats' in e:
        check_partials(c, part, e['stats'][0], 'statistics')


def run_bwd(ops, c, p, e):
    spec = ops.ConvSpec(c.cin, c.cout, c.k, c.stride, c.pad, c.dil)
    _, wb = ops.weight_prep(p.w.float().to(DEV), c.dtype, want_fwd=False)
    dy = g(cx.nhwc(p.dy), c.dtype)
    hw = (c.H, c.W)
    bits = gate_bits(ops, e, c.dtype) if 'gate' in e else None
    bn = lambda s='': (g(e['bn_x' + s], c.dtype), g(e['mean' + s], torch.float32), g(e['invstd' + s], torch.float32))
    parts = []
    if c.entry == 'bwd':
        dx = ops.conv2d_bwd_data(dy, wb, spec, hw)
    elif c.entry == 'bwd_addend':
        dx = ops.conv2d_bwd_data(dy, wb, spec, hw, addend=g(e['addend'], c.dtype))
    elif c.entry == 'bwd_addend_bits':
        dx = ops.conv2d_bwd_data(dy, wb, spec, hw, addend=g(e['addend'], c.dtype), addend_mask=bits)
    elif c.entry == 'bwd_bnstat':
        r = ops.conv2d_bwd_data_bnstat(dy, wb, spec, hw, bits, *bn())
        assert r is not None, 'shape not served'
        dx, parts = r[0], [r[1]]
    elif c.entry == 'bwd_addend_bnstat':
        r = ops.conv2d_bwd_data_addend_bnstat(dy, wb, spec, hw, g(e['addend'], c.dtype), bits, *bn())
        assert r is not None, 'shape not served'
        dx, parts = r[0], [r[1]]
    elif c.entry == 'bwd_addend_half':
        dx, none = ops.conv2d_bwd_data_addend_half(dy, wb, spec, hw, g(e['addend_half'], c.dtype))
        assert none is None
    elif c.entry == 'bwd_addend_half_stats':
        dx, part = ops.conv2d_bwd_data_addend_half(dy, wb, spec, hw, g(e['addend_half'], c.dtype), prev3=(bits, *bn()))
        assert part is not None, 'statistics not served'
        parts = [part]
    elif c.entry == 'bwd_addend_bnstat2':
        r = ops.conv2d_bwd_data_addend_bnstat2(dy, wb, spec, hw, g(e['addend'], c.dtype), bits, *bn(), *bn('2'))
        assert r is not None, 'shape not served'
        dx, parts = r[0], [r[1], r[2]]
    else:
        raise AssertionError(c.entry)
    assert torch.equal(dx.cpu(), cx.to_dtype(e['out'], c.dtype)), 'data gradient'
    assert len(parts) == len(e.get('stats', []))
    for i, part in enumerate(parts):
        check_partials(c, part, e['stats'][i], 'gated statistics %d' % i)


def run_wgrad(ops, c, p, e):
    spec = ops.ConvSpec(c.cin, c.cout, c.k, c.stride, c.pad, c.dil)
    x, dy = g(cx.nhwc(p.x), c.dtype), g(cx.nhwc(p.dy), c.dtype)
    x2 = None
    if c.c1:
        x, x2 = x[..., :c.c1].contiguous(), x[..., c.c1:].contiguous()
    ref = e['out'].to(torch.float32)
    if c.entry == 'wgrad':
        dw = ops.conv2d_bwd_weight(x, dy, spec, x2=x2)
    elif c.entry == 'wgrad_off':                           # a wider gradient tensor: this conv's channels at an offset, the others untouched
        wide = torch.full((c.cout, c.cin + 64, c.k, c.k), 7.0, device=DEV)
        ops.conv2d_bwd_weight(x, dy, spec, out=wide, out_ci_off=64)
        assert torch.equal(wide[:, :64].cpu(), torch.full((c.cout, 64, c.k, c.k), 7.0)), 'channels in front of the window were written'
        dw = wide[:, 64:]
    elif c.entry == 'wgrad_clip':                          # the parameter's own shape of a layer computed at padded channel counts
        dw = ops.conv2d_bwd_weight_clip(x, dy, spec, c.cout - 32, c.cin - 32)
        ref = ref[:c.cout - 32, :c.cin - 32]
    else:
        dw, db = ops.conv2d_bwd_weight_bias(x, dy, spec)
        L = _lib.lib()
        part = torch.empty((L.sl_conv2d_bwd_weight_bias_rows(C.byref(cx.desc(c)), 0, 0), c.cout), dtype=torch.float32, device=DEV)
        ws = ops.workspace(L.sl_conv2d_bwd_weight_workspace(C.byref(cx.desc(c))), x.device, 'wgrad')
        dw2 = torch.empty_like(dw)
        ops.check(L.sl_conv2d_bwd_weight_bias(C.byref(cx.desc(c)), ops._p(x), None, ops._p(dy), ops._p(dw2), ops._p(ws), ws.numel(), ops._p(part), ops._s()), 'bwd_weight_bias')
        assert torch.equal(part.double().sum(0).cpu(), e['bias']), 'bias partials summed in float64'
        assert torch.equal(db.double().cpu(), e['bias']) and torch.equal(dw2, dw), 'bias gradient'
    assert torch.equal(dw.cpu(), ref), 'weight gradient'


@pytest.mark.parametrize('c', cx.TABLE, ids=cx.IDS)
def test_conv_route_is_exact_on_integer_operands(hip, c):
    from segland_amd import ops
    assert cx.query(hip, c) == c.code, 'the case drifted to another kernel'
    p = cx.problem(c)
    e = cx.expected(c)
    rec = cx.check_bounds(c, e)
    print('%s: reference max |out| %g%s' % (cx.case_id(c), rec['max_out'], ', max partial %g' % rec['max_partial'] if 'max_partial' in rec else ''))
    for name, v in c.hooks:
        getattr(hip, name)(v)                              # (tests/conftest.py puts the record back after the test, also when it fails)
    (run_fwd, run_bwd, run_wgrad)[c.mode](ops, c, p, e)
