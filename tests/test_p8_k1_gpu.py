"""The 1x1 form of the half-tile kernel's K-tile body (conv_gemm_p8_kernel<EPI, K1 = true>) against the generic form it replaces on 1x1 launches
(test hook sl_debug_conv_p8_k1): same products, same order of sums -> every output and every statistic partial must be EQUAL BIT FOR BIT.  The forward is also
checked once against torch on the bf16-rounded operands at the bf16 kernel tolerance of test_kernels_gpu.py (2.5e-2 of the tensor scale)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
P8 = 5256256                 # sl_conv2d_tile_config code of conv_gemm_p8_kernel<bf16, 256, 256>
SL_EPI_STATS, SL_EPI_AFFINE, SL_EPI_GATE = 1, 2, 16

# B, H, W, Cin, Cout, stride.  At least 24 576 output rows (256-row tiles) and fewer than 65 536 (from there the pixel-stationary kernel takes K <= 256).
CASES = [
    (8, 64, 64, 512, 2048, 1),
    (8, 64, 64, 2048, 512, 1),
    (8, 64, 64, 1024, 256, 1),
    (8, 128, 128, 256, 512, 2),       # stride 2: forward only (the half-tile kernel serves data gradients of stride-1 convs)
    (7, 62, 63, 256, 256, 1),         # 27 342 rows = 106 tiles + 206 rows: the last tile's rows past M must read zeros (they are part of the column sums)
    (8, 64, 64, 64, 256, 1),          # forward nk = 1: only the last peeled K-tile runs
    (8, 64, 64, 128, 256, 1),         # forward nk = 2: the two peeled K-tiles without the steady loop
    (8, 64, 64, 256, 64, 1),          # data gradient nk = 1
    (8, 64, 64, 256, 128, 1),         # data gradient nk = 2
]


def _run(hip, ops, case, g):
    """Every p8 launch kind of the case -> list of (name, tensor)."""
    B, H, W, Cin, Cout, st = case
    dt = torch.bfloat16
    spec = ops.ConvSpec(Cin, Cout, 1, st, 0, 1)
    d = ops.conv_desc(dt, B, H, W, spec)
    Ho, Wo = spec.out_hw(H, W)
    x = torch.randn(B, H, W, Cin, generator=g).to(dt).to(DEV)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) * (3.0 / Cin) ** 0.5).to(dt).float().to(DEV)
    wf, wb = ops.weight_prep(w, dt)
    out = []
    if Cout % 256 == 0:
        assert hip.sl_conv2d_tile_config_ex(C.byref(d), 0, SL_EPI_STATS) == P8 and hip.sl_conv2d_tile_config_ex(C.byref(d), 0, SL_EPI_AFFINE) == P8, 'forward not on conv_gemm_p8_kernel'
        y, part = ops.conv2d_fwd(x, wf, spec, want_stats=True)                                   # <0>: store + statistic partials
        scale = (torch.rand(Cout, generator=g) + 0.5).to(DEV)
        shift = torch.randn(Cout, generator=g).to(DEV)
        res = torch.randn(B, Ho, Wo, Cout, generator=g).to(dt).to(DEV)
        ya = ops.conv2d_affine_fwd(x, wf, spec, scale, shift, residual=res, relu=True)           # <2>: affine store phase
        yb, _ = ops.conv2d_fwd(x, wf, spec, bias=shift, relu=True)
        out += [('forward', y), ('forward statistic partials', part), ('folded BN + residual + ReLU', ya), ('bias + ReLU', yb)]
    if Cin % 256 == 0 and st == 1:
        assert hip.sl_conv2d_tile_config_ex(C.byref(d), 1, 0) == P8 and hip.sl_conv2d_tile_config_ex(C.byref(d), 1, SL_EPI_GATE) == P8, 'data gradient not on conv_gemm_p8_kernel'
        dy = torch.randn(B, Ho, Wo, Cout, generator=g).to(dt).to(DEV)
        dx = ops.conv2d_bwd_data(dy, wb, spec, (H, W))                                           # <0>
        add = torch.randn(B, H, W, Cin, generator=g).to(dt).to(DEV)
        bits = torch.randint(0, 256, (add.numel() // 8,), dtype=torch.uint8, generator=g).to(DEV)
        dxa = ops.conv2d_bwd_data(dy, wb, spec, (H, W), addend=add, addend_mask=bits)
        c = (torch.randn(B, H, W, Cin, generator=g) * 2 + 0.5).to(dt).to(DEV)
        mean = (torch.randn(Cin, generator=g) * 0.3 + 0.5).to(DEV)
        invstd = (torch.rand(Cin, generator=g) + 0.5).to(DEV)
        out += [('data gradient', dx), ('data gradient + gated addend', dxa)]
        served = hip.sl_conv2d_bwd_data_bnstat_rows(C.byref(d)) > 0                              # the library offers the fused form on whole 256-row tiles only
        assert served or (B * H * W) % 256, 'gated data gradient with BN statistic partials not served'
        if served:
            gg, gpart = ops.conv2d_bwd_data_bnstat(dy, wb, spec, (H, W), bits, c, mean, invstd)    # <1>: gated store + BN-backward column sums
            out += [('gated data gradient', gg), ('BN-backward statistic partials', gpart)]
    assert out
    return x, w, out


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%dx%d_%d-%d_s%d' % c)
def test_p8_k1_equals_generic_bit_for_bit(hip, case):
    """Forward (+ statistic partials), affine forward, data gradient (+ gated addend), gated data gradient with BN statistic partials: K1 form (default) vs generic form
    (hook off) torch.equal; the forward against torch.nn.functional.conv2d in fp32 on the same bf16-rounded operands."""
    from segland_amd import ops
    B, H, W, Cin, Cout, st = case
    res = {}
    try:
        for on in (0, 1):
            hip.sl_debug_conv_p8_k1(on)
            g = torch.Generator(device='cpu').manual_seed(Cin * 7 + Cout + st)
            res[on] = _run(hip, ops, case, g)
            torch.cuda.synchronize()
    finally:
        hip.sl_debug_conv_p8_k1(1)
    x, w, new = res[1]
    for (name, a), (_, b) in zip(res[0][2], new):
        assert a.shape == b.shape and torch.equal(a, b), '%s: the 1x1 form differs from the generic form (%d elements)' % (name, int((a != b).sum()))
    if new[0][0] == 'forward':
        idx = [0, B // 2, B - 1]                                      # three images, the last one holds the ragged tile
        ref = F.conv2d(x[idx].float().permute(0, 3, 1, 2), w, None, st, 0, 1).permute(0, 2, 3, 1)
        got = new[0][1][idx].float()
        err, s = float((got - ref).abs().max()), float(ref.abs().max())
        print('%s forward vs torch: max abs err %.3g of scale %.3g' % (case, err, s))
        assert err <= 2.5e-2 * max(s, 1e-6), 'forward vs torch: max abs err %g vs scale %g' % (err, s)
