"""The fused data-gradient entries write exactly the partial rows their served-queries promise: the queries answer from the plan the launch runs (csrc/conv_gemm.hip
choose_kernel), so a buffer of the promised rows is filled completely and nothing behind it is touched, on every kernel family that has such a store phase."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 3              # rows behind the promised ones
ADDEND, GATE = 4, 16   # SL_EPI_* of include/segland_hip.h

ROUTES = {
    # name: (form, B or None = the smallest batch the family takes, H, W, Cin, Cout, k, stride, epilogue bits of the launch, family)
    'sk_gate_addend': ('addend_bnstat', 1, 256, 256, 128, 64, 1, 1, GATE | ADDEND, 6),          # pixel-stationary kernel, K = 64: 65 536 rows, one image
    'sk_dual': ('addend_bnstat2', 1, 256, 256, 128, 64, 1, 1, GATE | ADDEND, 6),
    'sk_half_gate': ('addend_half_gate', 1, 256, 256, 128, 64, 1, 1, GATE | ADDEND, 6),
    'sk_half': ('addend_half', 1, 256, 256, 128, 64, 1, 1, ADDEND, 6),
    'half_tile': ('bnstat', 1, 160, 160, 256, 512, 1, 1, GATE, 5),                              # 25 600 rows: the first 256-row-tile sizes
    'parity_planes': ('bnstat', 6, 128, 128, 128, 128, 3, 2, GATE, 4),                          # four planes of 24 576 rows on 256-row tiles
    'stride2_one_launch': ('bnstat', 1, 128, 128, 128, 128, 3, 2, GATE, 4),                     # the same layer, too few rows per plane: 128-row tiles
    'c64k3': ('bnstat', None, 128, 128, 64, 64, 3, 1, GATE, 7),
}


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_fused_data_gradient_fills_the_promised_partial_rows(hip, route):
    """Per route: the entry point called directly with a partial buffer of the promised rows + guard rows, all NaN beforehand -- every promised row is written and finite,
    the guard rows stay NaN, and dx is bit-identical to what the ops wrapper returns for the same inputs."""
    from segland_amd import ops
    form, B, H, W, cin, cout, k, stride, epi, family = ROUTES[route]
    dt_ = torch.bfloat16
    spec = ops.ConvSpec(cin, cout, k, stride, k // 2, 1)
    cfg = lambda b: hip.sl_conv2d_tile_config_ex(C.byref(ops.conv_desc(dt_, b, H, W, spec, None)), 1, epi)
    if B is None:
        B = next(b for b in range(1, 17) if cfg(b) // 1000000 == family)
    d = ops.conv_desc(dt_, B, H, W, spec, None)
    assert cfg(B) // 1000000 == family, cfg(B)
    rows = {'bnstat': hip.sl_conv2d_bwd_data_bnstat_rows, 'addend_half': hip.sl_conv2d_bwd_data_addend_half_ok}.get(form, hip.sl_conv2d_bwd_data_addend_bnstat_rows)(C.byref(d))
    assert rows > 0, 'shape not served'
    torch.manual_seed(7)
    w = torch.randn(cout, cin, k, k, device=DEV) * (1.0 / (k * k * cout)) ** 0.5
    _, wb = ops.weight_prep(w, dt_)
    dy = torch.randn(B, d.Ho, d.Wo, cout, device=DEV).to(dt_)
    bn_x, bn_x2, addend = (torch.randn(B, H, W, cin, device=DEV).to(dt_) for _ in range(3))
    half = torch.randn(B, H // 2, W // 2, cin, device=DEV).to(dt_)
    gate = torch.randint(0, 256, (B * H * W * cin // 8,), dtype=torch.uint8, device=DEV)
    (mean, invstd), (mean2, invstd2) = ((torch.randn(cin, device=DEV) * 0.1, torch.rand(cin, device=DEV) + 0.5) for _ in range(2))
    dx = torch.empty(B, H, W, cin, dtype=dt_, device=DEV)
    nbuf = 0 if form == 'addend_half' else (2 if form == 'addend_bnstat2' else 1)
    bufs = [torch.full((rows + GUARD, 2, cin), float('nan'), device=DEV) for _ in range(nbuf)]
    p, r, s = ops._p, C.byref(d), ops._s()
    if form == 'bnstat':
        rc = hip.sl_conv2d_bwd_data_bnstat(r, p(dy), p(wb), p(gate), p(bn_x), p(mean), p(invstd), p(dx), p(bufs[0]), s)
        want = ops.conv2d_bwd_data_bnstat(dy, wb, spec, (H, W), gate, bn_x, mean, invstd)
    elif form == 'addend_bnstat':
        rc = hip.sl_conv2d_bwd_data_addend_bnstat(r, p(dy), p(wb), p(addend), p(gate), p(bn_x), p(mean), p(invstd), p(dx), p(bufs[0]), s)
        want = ops.conv2d_bwd_data_addend_bnstat(dy, wb, spec, (H, W), addend, gate, bn_x, mean, invstd)
    elif form == 'addend_bnstat2':
        rc = hip.sl_conv2d_bwd_data_addend_bnstat2(r, p(dy), p(wb), p(addend), p(gate), p(bn_x), p(mean), p(invstd), p(bn_x2), p(mean2), p(invstd2), p(dx), p(bufs[0]), p(bufs[1]), s)
        want = ops.conv2d_bwd_data_addend_bnstat2(dy, wb, spec, (H, W), addend, gate, bn_x, mean, invstd, bn_x2, mean2, invstd2)
    elif form == 'addend_half_gate':
        rc = hip.sl_conv2d_bwd_data_addend_half(r, p(dy), p(wb), p(half), p(gate), p(bn_x), p(mean), p(invstd), p(dx), p(bufs[0]), s)
        want = ops.conv2d_bwd_data_addend_half(dy, wb, spec, (H, W), half, (gate, bn_x, mean, invstd))
    else:
        rc = hip.sl_conv2d_bwd_data_addend_half(r, p(dy), p(wb), p(half), None, None, None, None, p(dx), None, s)
        want = ops.conv2d_bwd_data_addend_half(dy, wb, spec, (H, W), half)
    ops.check(rc, route)
    assert want is not None, 'the wrapper did not take the fused form'
    assert all(t is not None for t in want[1:1 + nbuf]) and (nbuf or want[1] is None)
    torch.cuda.synchronize()
    print('%s: B %d, config %d, %d partial rows' % (route, B, cfg(B), rows))
    for buf, wpart in zip(bufs, want[1:]):
        assert wpart.shape == (rows, 2, cin)
        assert bool(torch.isfinite(buf[:rows]).all()), '%d of %d promised rows hold an unwritten or non-finite value' % (int((~torch.isfinite(buf[:rows])).any(2).any(1).sum()), rows)
        assert bool(torch.isnan(buf[rows:]).all()), 'rows behind the promised ones were written'
    assert torch.equal(dx, want[0]), 'dx of the direct call differs from the ops wrapper'
