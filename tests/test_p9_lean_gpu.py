"""The lean form of the 3x3 patch kernel's K-tile loop (conv_gemm_p9_kernel<EPI, D = 1 / 2 / 4, FLIP>) against the generic loop it replaces (D = 0; test hook
sl_debug_conv_p9_lean): same products, same order of sums -> every output and every statistic partial must be EQUAL BIT FOR BIT.  One d = 2 forward is also checked
against torch on the bf16-rounded operands at the bf16 kernel tolerance of test_kernels_gpu.py (2.5e-2 of the tensor scale).

Every case has 32 768 output rows, the kernel's lower limit.  The 64 x 64 maps have interior tiles as well as border tiles; on the 32 x 32 map with d = 4 every tile touches
the padding on at least two sides."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SL_EPI_STATS, SL_EPI_AFFINE, SL_EPI_GATE, SL_EPI_SPLITK = 1, 2, 16, 32
P9_SPLITK = 18256256         # sl_conv2d_tile_config code of a split-K launch on conv_gemm_p9_kernel

# B, H, W, Cin, Cout, dilation
CASES = [
    (8, 64, 64, 64, 256, 1),          # one chunk: the peeled last chunk alone; two patch buffers, never switched.  Forward only (the data gradient's N is 64)
    (8, 64, 64, 128, 256, 1),         # two chunks: patch buffer switch
    (8, 64, 64, 192, 256, 2),         # three chunks: the weight slot pairs change roles twice; single patch buffer with its refill.  Forward only
    (8, 64, 64, 256, 256, 2),         # data gradient and gated forms: flipped window
    (32, 32, 32, 256, 256, 4),        # every tile touches the padding on at least two sides
    (8, 64, 64, 256, 512, 4),         # two column tiles (forward), the column-group block order
]
TORCH_CASE = (8, 64, 64, 256, 256, 2)


def _fam8(hip, d, mode, epi, what):
    assert hip.sl_conv2d_tile_config_ex(C.byref(d), mode, epi) // 1000000 == 8, '%s not on conv_gemm_p9_kernel' % what


def _run(hip, ops, case, g):
    """Every patch-kernel launch kind of the case -> list of (name, tensor)."""
    B, H, W, Cin, Cout, dil = case
    dt = torch.bfloat16
    spec = ops.ConvSpec(Cin, Cout, 3, 1, dil, dil)
    d = ops.conv_desc(dt, B, H, W, spec)
    x = torch.randn(B, H, W, Cin, generator=g).to(dt).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (3.0 / (9 * Cin)) ** 0.5).to(dt).float().to(DEV)
    wf, wb = ops.weight_prep(w, dt)
    dy = torch.randn(B, H, W, Cout, generator=g).to(dt).to(DEV)
    bias_v = torch.randn(Cout, generator=g).to(DEV)
    scale_v = (torch.rand(Cout, generator=g) + 0.5).to(DEV)
    _fam8(hip, d, 0, SL_EPI_STATS, 'forward')
    _fam8(hip, d, 0, SL_EPI_AFFINE, 'affine forward')
    y, part = ops.conv2d_fwd(x, wf, spec, want_stats=True)
    yp, pp = ops.conv2d_fwd(x, wf, spec, pre_addend=dy, want_stats=True)                     # the shaped store phases of test_conv_3x3_patch_kernel
    yb, _ = ops.conv2d_fwd(x, wf, spec, bias=bias_v, relu=True)
    ya = ops.conv2d_affine_fwd(x, wf, spec, scale_v, bias_v, residual=dy, relu=True)
    out = [('forward', y), ('forward statistic partials', part), ('forward + pre-addend', yp), ('statistic partials with pre-addend', pp), ('bias + ReLU', yb),
           ('folded BN + residual + ReLU', ya)]
    if Cin % 256 == 0:
        _fam8(hip, d, 1, 0, 'data gradient')
        _fam8(hip, d, 1, SL_EPI_GATE, 'gated data gradient')
        dx = ops.conv2d_bwd_data(dy, wb, spec, (H, W))
        add = torch.randn(B, H, W, Cin, generator=g).to(dt).to(DEV)
        bits = torch.randint(0, 256, (add.numel() // 8,), dtype=torch.uint8, generator=g).to(DEV)
        dxa = ops.conv2d_bwd_data(dy, wb, spec, (H, W), addend=add, addend_mask=bits)
        c = (torch.randn(B, H, W, Cin, generator=g) * 2 + 0.5).to(dt).to(DEV)
        mean = (torch.randn(Cin, generator=g) * 0.3 + 0.5).to(DEV)
        invstd = (torch.rand(Cin, generator=g) + 0.5).to(DEV)
        out += [('data gradient', dx), ('data gradient + gated addend', dxa)]
        assert hip.sl_conv2d_bwd_data_bnstat_rows(C.byref(d)) > 0, 'gated data gradient with BN statistic partials not served'
        gg, gpart = ops.conv2d_bwd_data_bnstat(dy, wb, spec, (H, W), bits, c, mean, invstd)
        out += [('gated data gradient', gg), ('BN-backward statistic partials', gpart)]
    return x, w, out


def _both(hip, fn):
    """fn() under the generic loop (hook 0) and under the lean form (default) -> {0: ..., 1: ...}"""
    res = {}
    try:
        for on in (0, 1):
            hip.sl_debug_conv_p9_lean(on)
            res[on] = fn()
            torch.cuda.synchronize()
    finally:
        hip.sl_debug_conv_p9_lean(1)
    return res


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%dx%d_%d-%d_d%d' % c)
def test_p9_lean_equals_generic_bit_for_bit(hip, case):
    """Forward + statistic partials, the shaped store phases, data gradient (+ gated addend), gated data gradient with BN statistic partials: lean form (default) vs generic
    loop (hook off) torch.equal; the forward of the d = 2 case against torch.nn.functional.conv2d in fp32 on the same bf16-rounded operands."""
    from segland_amd import ops
    B, H, W, Cin, Cout, dil = case
    res = _both(hip, lambda: _run(hip, ops, case, torch.Generator(device='cpu').manual_seed(Cin * 7 + Cout + dil)))
    x, w, new = res[1]
    assert len(new) == (10 if Cin % 256 == 0 else 6)
    for (name, a), (_, b) in zip(res[0][2], new):
        assert a.shape == b.shape and torch.equal(a, b), '%s: the lean form differs from the generic loop (%d elements)' % (name, int((a != b).sum()))
    if case == TORCH_CASE:
        idx = [0, B - 1]
        ref = F.conv2d(x[idx].float().permute(0, 3, 1, 2), w, None, 1, dil, dil).permute(0, 2, 3, 1)
        got = new[0][1][idx].float()
        err, s = float((got - ref).abs().max()), float(ref.abs().max())
        print('%s forward vs torch: max abs err %.3g of scale %.3g' % (case, err, s))
        assert err <= 2.5e-2 * max(s, 1e-6), 'forward vs torch: max abs err %g vs scale %g' % (err, s)


def test_p9_lean_split_k_equals_generic_bit_for_bit(hip):
    """Split-K (the fine-tune pair's frozen 3x3 convs through conv2d_affine_fwd): 1152 input channels are 18 chunks in 4 parts that start at chunks 0, 4, 9 and 13 -- with
    d = 1 a part that starts at an odd chunk begins in the second patch buffer."""
    from segland_amd import ops
    B, H, W, Cin, Cout, dil = 2, 32, 32, 1152, 256, 1
    dt = torch.bfloat16
    spec = ops.ConvSpec(Cin, Cout, 3, 1, dil, dil)
    d = ops.conv_desc(dt, B, H, W, spec)
    assert hip.sl_conv2d_tile_config_ex(C.byref(d), 0, SL_EPI_AFFINE | SL_EPI_SPLITK) == P9_SPLITK, 'not a split-K launch on conv_gemm_p9_kernel'
    assert hip.sl_conv2d_affine_fwd_workspace(C.byref(d)) == 4 * B * H * W * Cout * 4, 'not four parts'
    g = torch.Generator(device='cpu').manual_seed(11)
    x = torch.randn(B, H, W, Cin, generator=g).to(dt).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (3.0 / (9 * Cin)) ** 0.5).to(dt).float().to(DEV)
    wf, _ = ops.weight_prep(w, dt)
    scale_v = (torch.rand(Cout, generator=g) + 0.5).to(DEV)
    bias_v = torch.randn(Cout, generator=g).to(DEV)
    res = _both(hip, lambda: ops.conv2d_affine_fwd(x, wf, spec, scale_v, bias_v, relu=True))
    assert torch.equal(res[0], res[1]), 'split-K: the lean form differs from the generic loop (%d elements)' % int((res[0] != res[1]).sum())
    ref = torch.relu(F.conv2d(x.float().permute(0, 3, 1, 2), w, None, 1, dil, dil).permute(0, 2, 3, 1) * scale_v + bias_v)
    err, s = float((res[1].float() - ref).abs().max()), float(ref.abs().max())
    print('split-K forward vs torch: max abs err %.3g of scale %.3g' % (err, s))
    assert err <= 2.5e-2 * max(s, 1e-6), 'split-K forward vs torch: max abs err %g vs scale %g' % (err, s)
