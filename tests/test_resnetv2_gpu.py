"""Deep-stem backbones (resnet50v2 / resnet101v2) on the GPU: the new stem kernels one by one, the stem and the full model against the golden records made from
the reference (tests/golden/g20..g22, tests/golden/make_golden_v2.py) and against the CPU restatement on this machine (tests/resnetv2_cpu.py), a bench-shaped
graphed step with its dispatch asserted, and the frozen fine-tune route.  Tolerances are those of the corresponding 7x7-stem / G5 / G6 / G7 tests."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import formula as fm
from oracle import pop_oracle as po
import resnetv2_cpu as rv
from test_kernels_gpu import assert_close, rnd
from test_model_gpu import GTOLS, TOLS, check, check_grad, nchw, nhwc, relerr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16]


# ------------------------------------------------------------------------------------------------ 1. pool kernels
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Cn,B,Hc,Wc', [(64, 2, 24, 40), (128, 2, 24, 40), (128, 3, 13, 22), (64, 1, 7, 9), (192, 2, 10, 6)])
def test_pool_kernels_exact(hip, dtype, Cn, B, Hc, Wc):
    """BN + ReLU + maxpool for C channels and its backward, no tolerance: values, first-maximum positions (many exact ties at zero behind the ReLU) and the routed
    gradient are bit-equal to torch on the same numbers; the BN-backward partials equal the stand-alone reduce pass; at C = 64 the old entry points give the same bytes."""
    from segland_amd import _lib, ops
    g = torch.Generator().manual_seed(Cn + Hc)
    c = (torch.randn(B, Hc, Wc, Cn, generator=g) * 8).round().clamp_(-32, 32) / 8
    c[torch.rand(B, Hc, Wc, Cn, generator=g) < 0.3] = 0.0
    # values on a 1/8 grid and scale / shift that keep the affine (and every sum of four gradients) exact in either dtype: what is compared is routing, not rounding
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (Cn,), generator=g)]
    shift = torch.tensor([0.0, 0.0, -0.25, 0.5])[torch.randint(0, 4, (Cn,), generator=g)]
    cg = c.to(DEV).to(dtype)
    pooled, idx = ops.stem_bn_relu_pool_c(cg, scale.to(DEV), shift.to(DEV), True)
    a = F.relu(c.permute(0, 3, 1, 2) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    a = rnd(a, dtype).requires_grad_(True)
    p_ref, i_ref = F.max_pool2d(a, 3, 2, 1, return_indices=True)
    assert torch.equal(nchw(pooled), p_ref.detach())
    # ATen's index is the flat position in the input plane; ours the window position ky*3+kx
    Hp, Wp = p_ref.shape[2:]
    py = torch.arange(Hp).view(1, 1, -1, 1); px = torch.arange(Wp).view(1, 1, 1, -1)
    mine = idx.cpu().permute(0, 3, 1, 2).long()
    flat = (2 * py - 1 + mine // 3) * Wc + (2 * px - 1 + mine % 3)
    assert torch.equal(flat, i_ref)
    gp = (torch.randn(p_ref.shape, generator=g) * 16).round().clamp_(-64, 64) / 16
    p_ref.backward(gp)
    mean = (torch.randn(Cn, generator=g) * 0.1).to(DEV); invstd = (0.5 + torch.rand(Cn, generator=g)).to(DEV)
    g0, part = ops.stem_pool_relu_bwd_bnstat_c(nhwc(gp, dtype), idx, cg, scale.to(DEV), shift.to(DEV), mean, invstd)
    assert part.shape[0] == hip.sl_stem_pool_relu_bwd_bnstat_c_rows(B, Hc, Wc, Cn)
    g_ref = a.grad * (a.detach() > 0)            # the masked pool gradient (d relu applied, the affine's scale is bn_bwd's business)
    assert torch.equal(nchw(g0), rnd(g_ref, dtype))
    # the partials: per channel against the fp64 sums over the STORED gradient and c3, at 1e-5 of sum |g| (the gate of the 7x7 stem's kernel, test_round5_gpu.py) ...
    rows = B * Hc * Wc
    g64, x64 = g0.double().reshape(-1, Cn), cg.double().reshape(-1, Cn)
    ref64 = torch.stack([g64.sum(0), (g64 * ((x64 - mean.double()) * invstd.double())).sum(0)])
    err = float(((part.double().sum(0) - ref64).abs() / (g64.abs().sum(0) + 1e-9)).max())
    print('pool bnstat C %d %s: column sums, max error relative to sum |g| %.2e' % (Cn, str(dtype)[6:], err))
    assert err < 1e-5, err
    # ... and against the stand-alone reduce pass on the same tensors, by the same gate
    ref_part = torch.empty((hip.sl_bn_bwd_reduce_rows(rows, Cn), 2, Cn), dtype=torch.float32, device=DEV)
    _lib.check(hip.sl_bn_bwd_reduce(ops.dt(cg), g0.data_ptr(), None, None, cg.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ref_part.data_ptr(), rows, Cn, ops._s()))
    torch.cuda.synchronize()
    err2 = float(((part.double().sum(0) - ref_part.double().sum(0)).abs() / (g64.abs().sum(0) + 1e-9)).max())
    assert err2 < 1e-5, err2
    if Cn == 64 and Hc % 2 == 0 and Wc % 2 == 0:
        p_old, i_old = ops.stem_bn_relu_pool(cg, scale.to(DEV), shift.to(DEV), True)
        g_old, part_old = ops.stem_pool_relu_bwd_bnstat(nhwc(gp, dtype), idx, cg, scale.to(DEV), shift.to(DEV), mean, invstd)
        assert torch.equal(p_old, pooled) and torch.equal(i_old, idx) and torch.equal(g_old, g0) and torch.equal(part_old, part)


# ------------------------------------------------------------------------------------------------ 2. conv1
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,W', [(2, 64, 64), (3, 50, 78), (2, 512, 512)])
def test_conv1_fwd_and_wgrad(hip, dtype, B, H, W):
    from segland_amd import ops
    img = fm.formula_image(B, H, W, 'stem3/img')
    w = fm.sym('stem3/w', (64, 3, 3, 3), (6.0 / 27) ** 0.5)
    imgr, wr = (rnd(img, dtype), rnd(w, dtype).requires_grad_(True))          # bf16: the fp32 result of bf16-rounded operands
    c_ref = F.conv2d(imgr, wr, None, 2, 1)
    c1, part = ops.stem3_conv_fwd(img.to(DEV), w.to(DEV), dtype, True)
    assert part.shape[0] == hip.sl_stem3_conv_stat_rows(B, H, W)
    assert_close(nchw(c1), c_ref, dtype, 'conv1')
    if dtype == torch.bfloat16:
        # the kernel multiplies bf16 hi + lo pairs of image and weights: against the UNROUNDED fp32 conv only the rounding of the stored output is left
        # (2^-9 of a value, i.e. at most 2e-3 of the scale; gate 4e-3).  With a lost lo term the operand rounding (2^-9 per factor over 27 taps) shows up here.
        c_full = F.conv2d(img, w, None, 2, 1)
        e = float((nchw(c1) - c_full).abs().max() / c_full.abs().max())
        print('conv1 bf16 vs unrounded fp32 conv: max error of scale %.2e' % e)
        assert e <= 4e-3, e
    s = part.sum(0).cpu()
    assert_close(s[0], c_ref.detach().sum((0, 2, 3)), dtype, 'stat sum', scale=float(c_ref.abs().sum((0, 2, 3)).max()))
    assert_close(s[1], (c_ref.detach() ** 2).sum((0, 2, 3)), dtype, 'stat sq')
    scale = (0.8 + 0.4 * fm.uniform01('stem3/sc', 64)).float(); shift = fm.sym('stem3/sh', (64,), 0.3)
    a1, none = ops.stem3_conv_fwd(img.to(DEV), w.to(DEV), dtype, False, scale.to(DEV), shift.to(DEV))
    assert none is None
    assert_close(nchw(a1), F.relu(c_ref.detach() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)), dtype, 'conv1 frozen form')
    gc = rnd(fm.sym('stem3/gc', tuple(c_ref.shape), 1.0), dtype)
    c_ref.backward(gc)
    dw = ops.stem3_conv_bwd_weight(img.to(DEV), nhwc(gc, dtype))
    assert_close(dw, wr.grad, dtype, 'conv1 wgrad')
    assert torch.equal(dw, ops.stem3_conv_bwd_weight(img.to(DEV), nhwc(gc, dtype))), 'weight gradient differs between two runs'


# ------------------------------------------------------------------------------------------------ 3. G20
def _stem_pair(dtype):
    from segland_amd.networks.backbones import get_backbone
    net = get_backbone(torch.nn.BatchNorm2d, backbone='resnet50v2', compute_dtype=dtype)
    ora = rv.DeepStemResNet((3, 4, 6, 3))
    sd = {k: fm.formula_tensor('g20/' + k, v) for k, v in ora.state_dict().items()}
    net.load_state_dict(sd); ora.load_state_dict(sd)
    return net.to(DEV), ora


@pytest.mark.parametrize('dtype', DTYPES)
def test_g20_stem(hip, dtype):
    from segland_amd.functional import flush_num_batches_tracked
    g = golden('g20_deep_stem')
    net, ora = _stem_pair(dtype)
    net.train(); ora.train()
    img = fm.formula_image(2, 64, 64, 'g20/img')
    y = net.forward_base_in(img.to(DEV))
    coef = fm.sym('g20/coef', (2, 128, 16, 16), 1.0)
    (y.float() * nhwc(coef, torch.float32)).sum().backward()
    flush_num_batches_tracked()
    tol = TOLS[dtype]
    fails = []

    def soft(fn, got, ref, t, what):            # every figure is printed and every gate evaluated before the test fails
        got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
        print('g20 %s %-12s %s %.3g (gate %.2g)' % (str(dtype)[6:], what, 'max error of scale' if fn is check else 'relative L2', relerr(got, ref) if fn is check else
                                                     float(np.linalg.norm((got - ref).ravel()) / np.linalg.norm(np.asarray(ref).ravel())), t))
        try:
            fn(got, ref, t, what)
        except AssertionError as e:
            fails.append(str(e))
    soft(check, nchw(y), g['y'], tol, 'y')
    for n in ('conv1', 'conv2', 'conv3'):
        soft(check_grad, getattr(net, n).weight.grad, g['d_%s_w' % n], GTOLS[dtype], 'd_%s_w' % n)
    for n in ('bn1', 'bn2', 'bn3'):
        bn = getattr(net, n)
        soft(check_grad, bn.weight.grad, g['d_%s_gamma' % n], GTOLS[dtype], 'd_%s_gamma' % n); soft(check_grad, bn.bias.grad, g['d_%s_beta' % n], GTOLS[dtype], 'd_%s_beta' % n)
        soft(check, bn.running_mean, g['rm_' + n], tol, 'rm_' + n); soft(check, bn.running_var, g['rv_' + n], tol, 'rv_' + n)
        assert int(bn.num_batches_tracked) == 1
    if dtype == torch.float32:                      # the restatement on THIS machine's CPU: the tolerances of G5's same-box comparison
        yo = ora.stem(img)
        (yo * coef).sum().backward()
        check(nchw(y), yo.detach().numpy(), 1e-5, 'y vs same-box restatement')
        check_grad(net.conv1.weight.grad, ora.conv1.weight.grad.numpy(), 1e-2, 'd_conv1_w vs same-box restatement')
        check_grad(net.conv3.weight.grad, ora.conv3.weight.grad.numpy(), 1e-2, 'd_conv3_w vs same-box restatement')
        check_grad(net.bn1.weight.grad, ora.bn1.weight.grad.numpy(), 1e-2, 'd_bn1_gamma vs same-box restatement')
        check(net.bn3.running_var, ora.bn3.running_var.numpy(), 1e-5, 'rv_bn3 vs same-box restatement')
    net.eval()
    with torch.no_grad():
        soft(check, nchw(net.forward_base_in(img.to(DEV))), g['y_eval'], tol, 'y_eval')
    assert not fails, fails


def test_base_forward_return_list(hip):
    net, _ = _stem_pair(torch.float32)
    net.eval()
    with torch.no_grad():
        img = fm.formula_image(1, 64, 64, 'g20/img').to(DEV)
        outs = net.base_forward(img, return_list=True)
        assert [tuple(o.shape) for o in outs] == [(1, 8, 8, 2048), (1, 8, 8, 1024), (1, 8, 8, 512), (1, 16, 16, 256)]
        assert torch.equal(outs[0], net.base_forward(img))


# ------------------------------------------------------------------------------------------------ 4. G21
def build(is_ft=False, n_novel=0, dtype=torch.float32, criterion=True, backbone='resnet50v2'):
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.networks.pspnet_pop import GFSS_Model
    m = GFSS_Model(n_base=7, criterion=OrthLoss(255) if criterion else None, is_ft=is_ft, n_novel=n_novel, backbone=backbone,
                   pretrained_model=None, dilated=True, os=8, compute_dtype=dtype)
    fm.load_formula_weights(m)
    return m.to(DEV)


def test_g21_full_r50v2_fp32(hip):
    """resnet50v2 PSPNet-POP, B 2, 512 x 512, fp32 parity mode: the gates of test_g6_full_r50_fp32."""
    g = golden('g21_full_r50v2')
    m = build(dtype=torch.float32).train()
    img = fm.formula_image(2, 512, 512, 'g6/img').to(DEV)
    mask = fm.formula_mask(2, 512, 512, 8, 'g6/mask').to(DEV)
    crit = m.criterion
    m.criterion = None
    logits = m(img)
    m.criterion = crit
    sb = F.normalize(m.base_emb.float(), dim=-1)
    d = crit(logits, mask, proto_sim=sb @ sb.t())
    d['total_loss'].backward()
    print('g21 logits max error of scale %.3g; losses %r' % (float(np.abs(logits.detach().cpu().numpy() - g['logits']).max() / np.abs(g['logits']).max()),
                                                             {k: float(v) for k, v in d.items()}))
    check(logits, g['logits'], 1e-3, 'logits (1e-3 rel fp32)')
    np.testing.assert_allclose(d['seg_loss'].item(), g['seg'], rtol=1e-4)
    np.testing.assert_allclose(d['orth_loss'].item(), g['orth'], rtol=1e-4)
    np.testing.assert_allclose(d['total_loss'].item(), g['total'], rtol=1e-4)
    gn = torch.nn.utils.clip_grad_norm_(m.parameters(), 1e30)
    np.testing.assert_allclose(gn.item(), g['gnorm'], rtol=5e-3)
    check_grad(m.base_emb.grad, g['d_base_emb'], 1e-2, 'd_base_emb')
    check_grad(m.classifier[4].weight.grad[0, :, 0, 0], g['d_cls4'], 1e-2, 'd_cls4')
    check_grad(m.decoder.bottleneck[3].bias.grad, g['d_dec_bias'], 1e-2, 'd_dec_bias')
    bb = m.backbone
    for k, w in (('d_conv1', bb.conv1.weight), ('d_conv2', bb.conv2.weight), ('d_conv3', bb.conv3.weight)):
        check_grad(w.grad, g[k], 5e-2, k + ' (end of the backward chain: every ReLU/maxpool kink on the way)')
    check_grad(bb.layer1[0].conv1.weight.grad[:, :, 0, 0], g['d_l1_conv1'], 5e-2, 'd_l1_conv1')
    check_grad(bb.layer1[0].downsample[0].weight.grad[:, :, 0, 0], g['d_l1_ds'], 5e-2, 'd_l1_ds')
    check(bb.bn1.running_mean, g['rm_bn1'], 1e-4, 'rm_bn1'); check(bb.bn1.running_var, g['rv_bn1'], 1e-4, 'rv_bn1')
    check(bb.bn3.running_mean, g['rm_bn3'], 1e-4, 'rm_bn3'); check(bb.bn3.running_var, g['rv_bn3'], 1e-4, 'rv_bn3')
    check(bb.layer4[2].bn3.running_mean, g['rm_l4'], 1e-3, 'rm_l4')
    assert int(bb.bn3.num_batches_tracked) == 1
    names = [str(k) for k in g['grad_norm_keys']]
    mine = dict(m.named_parameters())
    worst = max(abs(mine[k].grad.norm().item() - v) / max(v, 1e-6 * g['gnorm']) for k, v in zip(names, g['grad_norms']) if v > 1e-4 * g['gnorm'])
    assert worst < 2e-2, 'worst per-parameter grad-norm deviation %.3g' % worst
    # argmax: against the restatement on this machine (expected 0 differing pixels); any differing pixel must lie inside the top-two margin G6's test allows
    from segland_amd import ops
    am = ops.upsample_argmax(logits.detach().contiguous(), (512, 512)).cpu().numpy()
    ora = fm.load_formula_weights(rv.PopV2(n_base=7, criterion=None)).train()
    with torch.no_grad():
        lo = ora(img.cpu())
    up = F.interpolate(lo, size=(512, 512), mode='bilinear', align_corners=True)
    top2 = up.topk(2, dim=1).values
    margin = (top2[:, 0] - top2[:, 1]).numpy()
    diff = am != up.argmax(1).numpy()
    scale = float(np.abs(g['logits']).max())
    print('parity: g21 argmax differs from the same-box restatement on %d of %d pixels' % (int(diff.sum()), diff.size))
    assert (diff & (margin > 2e-3 * scale)).sum() == 0, 'argmax differs on %d clearly-separated pixels' % (diff & (margin > 2e-3 * scale)).sum()
    gd = am != g['argmax']
    assert gd.mean() < 2e-3, 'argmax differs from the golden record on %.4f of the pixels' % gd.mean()
    m.eval()
    with torch.no_grad():
        check(m(img), g['logits_eval'], 1e-3, 'logits_eval')


def test_g21_full_r50v2_bf16_eval(hip):
    """The gates of test_g6_full_r50_bf16_eval: 5 % of the logit scale, >= 98 % argmax agreement at feature resolution."""
    g = golden('g21_full_r50v2')
    m32 = build(dtype=torch.float32, criterion=False).train()
    img = fm.formula_image(2, 512, 512, 'g6/img').to(DEV)
    with torch.no_grad():
        m32(img)
    m = build(dtype=torch.bfloat16, criterion=False)
    m.load_state_dict(m32.state_dict())
    m.eval()
    with torch.no_grad():
        logits = m(img)
    check(logits, g['logits_eval'], 0.05, 'bf16 eval logits')
    agree = (logits.argmax(1).cpu().numpy() == g['logits_eval'].argmax(1)).mean()
    assert agree > 0.98, agree


# ------------------------------------------------------------------------------------------------ 5. bench shape
def _desc(B, H, W, cin, cout, k, pad):
    from segland_amd import _lib
    return _lib.SlConvDesc(_lib.SL_BF16, B, H, W, cin, cout, k, k, 1, pad, 1, H, W, cin)


def test_bench_shape_graphed_step(hip):
    """B 16, 512 x 512, bf16: the train step is captured by GraphedStep and replayed; two replays give bit-identical losses, gradients are finite, and the deep stem's
    conv layers run where the dispatch is expected to send them at 1 048 576 rows.  conv2 / conv3 at that size are also compared image by image with a batch-of-one
    launch (the index arithmetic at the far end of the tensor)."""
    import psutil
    avail = psutil.virtual_memory().available / 2 ** 30
    if avail < 56:
        pytest.skip('bench-shaped step: %.0f GB of host memory available, 56 wanted (the bound of test_c2_train_mode_bf16_gate[512])' % avail)
    from segland_amd import graph_step, ops
    from segland_amd.functional import prepared, spec_of
    STATS, AFFINE = 1, 2
    fam = lambda d, mode, epi: hip.sl_conv2d_tile_config_ex(C.byref(d), mode, epi)
    d2, d3 = _desc(16, 256, 256, 64, 64, 3, 1), _desc(16, 256, 256, 64, 128, 3, 1)
    assert fam(d2, 0, STATS) == 7016016 and fam(d2, 1, 0) == 7016016 and hip.sl_conv2d_wgrad_config(C.byref(d2)) == 1      # the 64 -> 64 3x3 patch kernel, both ways
    assert hip.sl_conv2d_stat_rows(C.byref(d2)) == 16 * 16 * 16
    assert fam(d3, 0, STATS) == 4256128 and hip.sl_conv2d_wgrad_config(C.byref(d3)) == 3 and hip.sl_conv2d_stat_rows(C.byref(d3)) == 4096      # ring tiles, nine-tap weight gradient
    assert fam(_desc(16, 128, 128, 128, 64, 1, 0), 0, STATS) == 6256064 and fam(_desc(16, 128, 128, 128, 256, 1, 0), 0, STATS) == 6256064   # layer1.0 conv1 / downsample: pixel-stationary
    m = build(dtype=torch.bfloat16).train()
    img = fm.formula_image(16, 512, 512, 'v2bench/img').to(DEV)
    mask = fm.formula_mask(16, 512, 512, 8, 'v2bench/mask').to(DEV)

    def body(img, mask):
        grads = [p.grad for p in m.parameters() if p.grad is not None]
        if grads:
            torch._foreach_zero_(grads)
        d = m(img, mask)
        d['total_loss'].backward()
        return d
    gs = graph_step.GraphedStep(body, m, None, warmup=1)
    gs(img, mask)
    gs(img, mask)                               # captured here
    a = {k: v.clone() for k, v in gs(img, mask).items()}
    b = {k: v.clone() for k, v in gs(img, mask).items()}
    torch.cuda.synchronize()
    assert gs.replays >= 2 and gs.failures == 0, (gs.replays, gs.failures)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.isfinite(a[k]).all(), (k, a[k], b[k])
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    assert m.backbone.conv1.weight.grad is not None and m.backbone.conv3.weight.grad.abs().sum() > 0
    # conv2 / conv3 forward at 16 x 256 x 256 rows against the same layer on the last image alone
    del gs
    bb = m.backbone
    x = torch.randn(16, 256, 256, 64, device=DEV).relu_().to(torch.bfloat16)
    for conv in (bb.conv2, bb.conv3):
        wf, wb = prepared(conv.weight, torch.bfloat16)
        y, _ = ops.conv2d_fwd(x, wf, spec_of(conv), want_stats=True)
        y1, _ = ops.conv2d_fwd(x[15:].contiguous(), wf, spec_of(conv), want_stats=True)
        assert_close(y[15:], y1, torch.bfloat16, 'forward of the last image')
        dx = ops.conv2d_bwd_data(y, wb, spec_of(conv), (256, 256))
        dx1 = ops.conv2d_bwd_data(y[15:].contiguous(), wb, spec_of(conv), (256, 256))
        assert_close(dx[15:], dx1, torch.bfloat16, 'data gradient of the last image')
        # the weight gradient over all 1 048 576 rows against the fp32 sum of sixteen one-image launches (fp32 accumulation both ways: the fp32 kernel tolerance x 10 for the
        # different summation trees over a million terms)
        dw = ops.conv2d_bwd_weight(x, y, spec_of(conv))
        dws = sum(ops.conv2d_bwd_weight(x[i:i + 1].contiguous(), y[i:i + 1].contiguous(), spec_of(conv)).double() for i in range(16))
        assert_close(dw, dws.float(), torch.float32, 'weight gradient at 16 x 256 x 256 rows', factor=10)


# ------------------------------------------------------------------------------------------------ 6. frozen route
def test_ft_frozen_route(hip):
    """ft_freeze() model (is_ft, 4 novel classes): one forward_novel step in fp32 mode against G22 (made from the reference) at the gates of test_g7_ft_fp32: the
    pseudo-label map equals the record up to numerically tied pixels (the bound of that test), losses, gradients, training and eval-mode logits; backbone parameters get no gradient."""
    g = golden('g22_ft_v2')
    m = build(True, 4, dtype=torch.float32)
    m.init_cls_n()
    with torch.no_grad():
        for k, p in m.classifier_n.named_parameters():
            p.add_(fm.sym('g7/cn/' + k, tuple(p.shape), 0.01).to(DEV))
    img = fm.formula_image(1, 512, 512, 'g7/img').to(DEV); img_b = fm.formula_image(1, 512, 512, 'g7/img_b').to(DEV)
    mask = fm.formula_mask(1, 512, 512, 4, 'g7/mask', ignore_rows=0, lo=8); mask[mask == 8] = 255
    mask_b = fm.formula_mask(1, 512, 512, 8, 'g7/mask_b', ignore_rows=0)
    mask, mask_b = mask.to(DEV), mask_b.to(DEV)
    m.train_mode()
    d = m(img, mask, img_b, mask_b)
    d['total_loss'].backward()
    mb = mask_b.cpu().numpy().astype(np.uint8)
    nd = int((mb != g['mask_b_new']).sum())
    print('parity: g22 pseudo labels differ on %d pixels' % nd)
    assert nd <= 8, 'pseudo labels differ on %d pixels' % nd
    np.testing.assert_allclose(d['seg_loss'].item(), g['seg'], rtol=2e-4)
    np.testing.assert_allclose(d['orth_loss'].item(), g['orth'], rtol=1e-4)
    check_grad(m.novel_emb.grad, g['d_novel_emb'], 5e-3, 'd_novel_emb')
    check_grad(m.classifier_n[4].weight.grad[0, :, 0, 0], g['d_clsn4'], 5e-3, 'd_clsn4')
    check_grad(m.classifier_n[0].weight.grad[::8, ::8, 0, 0], g['d_clsn0'], 5e-3, 'd_clsn0')
    assert all(p.grad is None for p in m.backbone.parameters()) and m.base_emb.grad is None and m.classifier[0].weight.grad is None
    crit = m.criterion
    m.criterion = None
    with torch.no_grad():
        preds = m(img, mask, img_b, fm.formula_mask(1, 512, 512, 8, 'g7/mask_b', ignore_rows=0).to(DEV))
    check(preds, g['preds'], 1e-3, 'preds')
    m.eval()
    with torch.no_grad():
        check(m(img), g['preds_all'], 1e-3, 'preds_all')
    # the bf16 frozen route runs (folded conv1, affine conv2, pool with bn3)
    mb16 = build(True, 4, dtype=torch.bfloat16, criterion=False)
    mb16.eval()
    with torch.no_grad():
        out = mb16(img)
    assert torch.isfinite(out).all() and out.shape[1] == 12
