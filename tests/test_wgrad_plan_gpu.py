"""Every route of the weight-gradient plan (csrc/conv_wgrad.hip plan_wgrad) writes exactly the bias-gradient partial rows sl_conv2d_bwd_weight_bias_rows promises, through
the C ABI on the shapes tests/test_abi_cpu.py pins: the smallest each route accepts.  Tolerances as test_round5_gpu.py::test_bias_gradient_inside_the_weight_gradient_kernel."""
import ctypes as C

import pytest
import torch

from test_abi_cpu import WGRAD_PLAN, _desc
from test_round5_gpu import close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD, UNWRITTEN = 12345.0, -7777.0


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _partials(rows, cout):
    """The promised rows (a value no column sum takes, so an unwritten row shows in the sum) and one guard row behind them."""
    part = torch.full((rows + 1, cout), UNWRITTEN, device=DEV)
    part[rows] = GUARD
    return part


def _check_partials(part, rows, dy, tol, what):
    assert bool((part[rows] == GUARD).all()), '%s: the row behind the %d promised rows was written' % (what, rows)
    close(part[:rows].sum(0), dy.float().reshape(-1, dy.shape[-1]).sum(0), 'bias gradient, %s' % what, tol=tol)


@pytest.mark.parametrize('case', WGRAD_PLAN, ids=lambda c: '%s-%dx%dx%d-%d-%d-k%d%s' % (('f32', 'bf16')[c[0]], *c[1], c[2], c[3], c[4], '-' + c[5] if c[5] else ''))
def test_every_route_writes_the_partial_rows_it_promises(hip, case):
    from segland_amd import _lib
    dtype, (B, H, W), cin, cout, k, hook, (code, rows_full, _, _) = case
    dt_ = torch.bfloat16 if dtype == _lib.SL_BF16 else torch.float32
    btol, wtol = (1e-5, 2.5e-2) if dt_ == torch.bfloat16 else (2e-5, 1e-4)
    M = B * H * W
    torch.manual_seed(cin + cout + k)
    x = torch.randn(B, H, W, cin, device=DEV).to(dt_)
    dy = (torch.randn(B, H, W, cout, device=DEV) + 0.25).to(dt_)
    d = _desc(dtype, B, H, W, cin, cout, k, 1, k // 2, 1)
    r = C.byref(d)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if hook:
        getattr(hip, hook)(0)
    assert hip.sl_conv2d_wgrad_config(r) == code
    ws = torch.empty(max(hip.sl_conv2d_bwd_weight_workspace(r), 1), dtype=torch.uint8, device=DEV)

    def check(rc):
        assert rc == 0, hip.sl_last_error_string()

    # the plain call: dw against fp32 torch, the promised rows sum to the bias gradient, nothing behind them is touched
    rows = hip.sl_conv2d_bwd_weight_bias_rows(r, 0, 0)
    assert rows == rows_full
    dw, part = torch.full((cout, cin, k, k), 7.0, device=DEV), _partials(rows, cout)
    check(hip.sl_conv2d_bwd_weight_bias(r, _p(x), None, _p(dy), _p(dw), _p(ws), ws.numel(), _p(part), st))
    _check_partials(part, rows, dy, btol, 'plain call')
    if k == 1:
        ref = (dy.float().reshape(M, cout).t() @ x.float().reshape(M, cin)).reshape(cout, cin, 1, 1)
    else:
        ref = torch.nn.grad.conv2d_weight(x.float().cpu().permute(0, 3, 1, 2), (cout, cin, k, k), dy.float().cpu().permute(0, 3, 1, 2), stride=1, padding=k // 2)
    close(dw, ref, 'weight gradient', tol=wtol)

    if (cin, cout, k) == (128, 384, 1):
        # zero-padded channel counts, and the same with the slab reduce deferred: the same route, so the same bits
        nv, cv = 288, 96
        rows_c = hip.sl_conv2d_bwd_weight_bias_rows(r, nv, cv)
        dwc, partc = torch.full((nv, cv, 1, 1), 7.0, device=DEV), _partials(rows_c, cout)
        check(hip.sl_conv2d_bwd_weight_clip(r, _p(x), None, _p(dy), _p(dwc), nv, cv, _p(ws), ws.numel(), _p(partc), st))
        _check_partials(partc, rows_c, dy, btol, 'clipped call')
        assert rows_c == rows and torch.equal(partc, part) and torch.equal(dwc, dw[:nv, :cv])
        dwd, partd, item = torch.full((nv, cv, 1, 1), 7.0, device=DEV), _partials(rows_c, cout), _lib.SlWgradReduce()
        check(hip.sl_conv2d_bwd_weight_defer(r, _p(x), None, _p(dy), _p(dwd), nv, cv, _p(ws), ws.numel(), _p(partd), C.byref(item), st))
        assert item.splits > 0, 'a 1x1 layer on the tile kernels leaves its flat slab reduce to the batch'
        check(hip.sl_wgrad_reduce_multi((_lib.SlWgradReduce * 1)(item), 1, st))
        _check_partials(partd, rows_c, dy, btol, 'deferred reduce')
        assert torch.equal(partd, part) and torch.equal(dwd, dwc)
    if (cin, cout, k) == (128, 128, 3):
        # into a wider dw: still the nine-tap kernel
        wide = torch.full((cout, 256, 3, 3), 7.0, device=DEV)
        check(hip.sl_conv2d_bwd_weight_ex(r, _p(x), None, _p(dy), _p(wide), 256, 128, _p(ws), ws.numel(), st))
        assert torch.equal(wide[:, 128:], dw) and bool((wide[:, :128] == 7).all())
        # clipped to (96, 96) the call leaves the nine-tap route for the tile kernels: another summation order, the same promise
        rows_c = hip.sl_conv2d_bwd_weight_bias_rows(r, 96, 96)
        dwc, partc = torch.full((96, 96, 3, 3), 7.0, device=DEV), _partials(rows_c, cout)
        check(hip.sl_conv2d_bwd_weight_clip(r, _p(x), None, _p(dy), _p(dwc), 96, 96, _p(ws), ws.numel(), _p(partc), st))
        _check_partials(partc, rows_c, dy, btol, 'clipped call (tile kernels)')
        close(dwc, ref[:96, :96], 'weight gradient, clipped', tol=wtol)
    torch.cuda.synchronize()
