"""Hybrid cross-entropy + multiclass soft Dice in the fused upsample + loss kernels (csrc/loss.hip, sl_upsample_ce_dice_fwd / _finalize / _bwd) against the definition in
torch, fp32 on the CPU of this machine:

    up = F.interpolate(preds, (H, W), bilinear, align_corners=True);  p = softmax(up);  over the valid pixels (label != ignore) of sample b
    I = sum p_c [t == c],  P = sum p_c,  T = sum [t == c];   dice = mean_b sum_c w_c (1 - (2 I + s) / (P + T + s));   ce = F.cross_entropy(up, target, w, ignore, eps)

every kernel (forward, finalize, gather / tiled / channel-sliced tiled backward, both per-thread widths), OrthLoss, the PSPNet-POP model in base and fine-tune mode and a
captured training step.  Without the hybrid entry points every test here fails (missing attribute / unexpected keyword)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import formula as fm

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GS = 0.7                         # upstream gradient
# the shapes of test_weighted_ce_gpu.CE_CASES: both per-thread widths (16, 33), one / two / three channel slices of the wide tiled backward, a ragged map, the identity scale
CE_CASES = [(8, (8, 8), (64, 64)), (12, (9, 7), (40, 33)), (21, (9, 7), (40, 33)), (33, (8, 8), (64, 64)), (33, (8, 8), (8, 8))]
MODES = {'plain': (False, 0.0), 'weights': (True, 0.0), 'weights+smoothing': (True, 0.1)}


def class_weights(K):
    """[0.5, 2] with one class at 0"""
    w = 1.25 + fm.sym('dice/w%d' % K, (K,), 0.75)
    w[K // 2] = 0.0
    return w


def torch_dice(up, target, w, s, ignore=255):
    """the Dice term of the definition on upsampled logits `up` [B, K, H, W]"""
    K = up.shape[1]
    p = up.softmax(1)
    valid = target != ignore
    oh = F.one_hot(target.masked_fill(~valid, 0), K).permute(0, 3, 1, 2).to(up.dtype) * valid[:, None]
    pm = p * valid[:, None]
    I, P, T = (pm * oh).sum((2, 3)), pm.sum((2, 3)), oh.sum((2, 3))
    d = 1 - (2 * I + s) / (P + T + s)
    return (d * (w.to(up.dtype) if w is not None else 1)).sum(1).mean()


def torch_hybrid(preds, target, HW, w, eps, s, lam, dtype):
    """(ce, dice, d (GS * (ce + lam * dice)) / d preds) of the definition in `dtype`"""
    pr = preds.to(dtype).clone().requires_grad_(True)
    up = F.interpolate(pr, size=HW, mode='bilinear', align_corners=True)
    dice = torch_dice(up, target, w, s)
    ce = F.cross_entropy(up, target, weight=None if w is None else w.to(dtype), ignore_index=255, label_smoothing=eps)
    ((ce + lam * dice) * GS).backward()
    return float(ce.detach()), float(dice.detach()), pr.grad.numpy()


@functools.lru_cache(maxsize=None)
def reference(K, hw, HW, weighted, eps, blank1=False, lam=1.0, s=1.0):
    preds = fm.sym('dice/p%d' % K, (2, K) + hw, 3.0)
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='dice/m%d' % K, block=8, ignore_rows=5)
    if blank1:
        target = torch.cat([target[:1], torch.full_like(target[1:], 255)])
    w = class_weights(K) if weighted else None
    ce, dice, dref = torch_hybrid(preds, target, HW, w, eps, s, lam, torch.float32)
    ce64, dice64, dref64 = torch_hybrid(preds, target, HW, w, eps, s, lam, torch.float64)
    valid = target[target != 255]
    wsum = float((w.double()[valid]).sum()) if weighted else float(valid.numel())
    oracle_grad_err = float(np.abs(dref - dref64).max())
    # the larger of the weighted test's floor (2e-8 scaled by how far weighting can raise a pixel's share of the mean) and 8 x the oracle's own fp32 error on this gradient
    # (margin for the kernels' other summation order and one more fp32 rounding in the coefficients; from the oracle alone)
    atol = max(2e-8 * (float(w.max()) if weighted else 1.0) * valid.numel() / wsum, 8.0 * oracle_grad_err)
    return dict(preds=preds, target=target, w=w, ce=ce, dice=dice, dref=dref, wsum=wsum, atol=atol, lam=lam, s=s,
                oracle_ce_err=abs(ce - ce64) / abs(ce64), oracle_dice_err=abs(dice - dice64) / abs(dice64), oracle_grad_err=oracle_grad_err)


def run_kernels(r, eps):
    """forward + finalize and backward twice each: two runs must give the same bits"""
    from segland_amd import ops
    pg, tg = r['preds'].to(DEV), r['target'].to(DEV)
    wg = None if r['w'] is None else r['w'].to(DEV)
    gs = torch.tensor([GS, GS * r['lam']], device=DEV)
    out, coef = ops.upsample_ce_dice_fwd(pg, tg, 255, weight=wg, label_smoothing=eps, smooth=r['s'])
    out2, coef2 = ops.upsample_ce_dice_fwd(pg, tg, 255, weight=wg, label_smoothing=eps, smooth=r['s'])
    dl = ops.upsample_ce_dice_bwd(pg, tg, out, coef, gs, 255, weight=wg, label_smoothing=eps)
    dl2 = ops.upsample_ce_dice_bwd(pg, tg, out, coef, gs, 255, weight=wg, label_smoothing=eps)
    assert tuple(out.shape) == (3,) and tuple(coef.shape) == tuple(pg.shape[:2]) + (2,)
    assert torch.equal(out, out2) and torch.equal(coef, coef2) and torch.equal(dl, dl2), 'run to run'
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(coef).all())
    return out.cpu(), dl.cpu().numpy()


def check_against(r, out, dl, what):
    print('%s: ce %.8g (torch %.8g, torch fp32 is %.2g relative from float64), dice %.8g (torch %.8g, %.2g from float64), weight sum %.8g (float64 %.8g)'
          % (what, out[0].item(), r['ce'], r['oracle_ce_err'], out[2].item(), r['dice'], r['oracle_dice_err'], out[1].item(), r['wsum']))
    print('   gradient: max abs error %.3g, floor %.3g (max |grad| %.3g; torch fp32 is %.2g absolute from float64)'
          % (float(np.abs(dl - r['dref']).max()), r['atol'], float(np.abs(r['dref']).max()), r['oracle_grad_err']))
    np.testing.assert_allclose(out[0].item(), r['ce'], rtol=2e-5)
    np.testing.assert_allclose(out[2].item(), r['dice'], rtol=2e-5)
    np.testing.assert_allclose(out[1].item(), r['wsum'], rtol=2e-5)
    np.testing.assert_allclose(dl, r['dref'], rtol=1e-3, atol=r['atol'])


# --------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_ce_dice_kernels(hip, K, hw, HW, mode, route):
    """ce and dice rtol 2e-5 each against torch fp32 (the bound of test_wide_head_gpu.test_upsample_ce_wide); gradient of 0.7 * (ce + dice) rtol 1e-3 with an absolute
    floor, the larger of 2e-8 * max(w) * n_valid / sum_p w_t and 8 x max |torch fp32 - torch float64| of the same gradient.  The two samples differ (rows 0..4 of sample 0
    are ignored and the label maps are independent), so sums pooled over the batch would miss.  Both distances are printed beside each result."""
    weighted, eps = MODES[mode]
    r = reference(K, hw, HW, weighted, eps)
    assert HW == (8, 8) or len(r['target'].unique()) == K + 1         # every class occurs, the zero-weight one too (an 8 x 8 label map has one block)
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl = run_kernels(r, eps)
    check_against(r, out, dl, 'K %d %s -> %s, %s, %s backward' % (K, hw, HW, mode, route))


@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('mode', ['plain', 'weights+smoothing'])
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_a_fully_ignored_sample_has_dice_zero_and_a_zero_gradient(hip, K, hw, HW, mode, route):
    """Sample 1 is entirely `ignore`: the same bounds against the oracle (whose Dice term of that sample is (1 - s / s) = 0), and dlogits[1] is exactly zero."""
    weighted, eps = MODES[mode]
    r = reference(K, hw, HW, weighted, eps, blank1=True)
    assert not r['dref'][1].any()
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl = run_kernels(r, eps)
    check_against(r, out, dl, 'K %d %s -> %s, sample 1 ignored, %s, %s backward' % (K, hw, HW, mode, route))
    assert not dl[1].any(), 'gradient of a sample without a valid pixel'
    assert np.abs(dl[0]).max() > 0


@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('K,hw,HW', [CE_CASES[0], CE_CASES[2]])
def test_the_two_upstream_scales_and_the_smooth_term(hip, K, hw, HW, route):
    """gscale = (0.7, 0.7 * 0.25) and smooth = 2.5: the gradient of 0.7 * (ce + 0.25 * dice) with that smooth, same bounds (catches swapped scales and a fixed smooth)"""
    r = reference(K, hw, HW, True, 0.1, lam=0.25, s=2.5)
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl = run_kernels(r, 0.1)
    check_against(r, out, dl, 'K %d %s -> %s, lambda 0.25, smooth 2.5, %s backward' % (K, hw, HW, route))


def test_out_of_range_labels_count_as_ignored(hip):
    """labels outside [0, K) enter neither term, as in the plain kernels: 250 in the place of some labels gives the results of 255 there"""
    from segland_amd import ops
    r = reference(8, (8, 8), (64, 64), True, 0.1)
    pg, wg = r['preds'].to(DEV), r['w'].to(DEV)
    t255 = r['target'].clone()
    t255[1, 10:20, 7:50] = 255
    t250 = t255.clone()
    t250[1, 10:20, 7:50] = 250
    t250[1, 12, 9] = -3
    gs = torch.tensor([GS, GS], device=DEV)
    res = []
    for t in (t255, t250):
        out, coef = ops.upsample_ce_dice_fwd(pg, t.to(DEV), 255, weight=wg, label_smoothing=0.1)
        res.append((out, coef, ops.upsample_ce_dice_bwd(pg, t.to(DEV), out, coef, gs, 255, weight=wg, label_smoothing=0.1)))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_ops_refuse_bad_arguments(hip):
    from segland_amd import ops
    r = reference(8, (8, 8), (64, 64), False, 0.0)
    pg, tg = r['preds'].to(DEV), r['target'].to(DEV)
    with pytest.raises(ValueError, match='7 class weights for 8 logit channels'):
        ops.upsample_ce_dice_fwd(pg, tg, 255, weight=torch.ones(7, device=DEV))
    with pytest.raises(RuntimeError, match='label_smoothing'):
        ops.upsample_ce_dice_fwd(pg, tg, 255, label_smoothing=1.5)
    with pytest.raises(RuntimeError, match='smooth'):
        ops.upsample_ce_dice_fwd(pg, tg, 255, smooth=0.0)
    out, coef = ops.upsample_ce_dice_fwd(pg, tg, 255)
    with pytest.raises(ValueError, match='two upstream gradients'):
        ops.upsample_ce_dice_bwd(pg, tg, out, coef, torch.ones(1, device=DEV), 255)


# --------------------------------------------------------------------------------------------- 2. OrthLoss
def test_dice_weight_zero_is_the_path_without_it(hip):
    """OrthLoss(255, dice_weight=0.0) and OrthLoss(255): the same keys, torch.equal values and gradients"""
    from segland_amd.loss.criterion import OrthLoss
    preds, aux = fm.sym('dice/ol/preds', (2, 8, 8, 8), 2.0), fm.sym('dice/ol/aux', (2, 8, 16, 16), 1.5)
    target = fm.formula_mask(2, 64, 64, 8, tag='dice/ol/mask', block=8, ignore_rows=7).to(DEV)
    sim = fm.sym('dice/ol/sim', (4, 11), 1.0).to(DEV)
    res = []
    for crit in (OrthLoss(255, dice_weight=0.0).to(DEV), OrthLoss(255).to(DEV)):
        pg, ag = preds.to(DEV).requires_grad_(True), aux.to(DEV).requires_grad_(True)
        d = crit(pg, target, is_ft=True, proto_sim=sim, aux_preds=ag)
        d['total_loss'].backward()
        res.append((d, pg.grad, ag.grad))
    assert list(res[0][0]) == list(res[1][0]) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss']
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_orth_loss_hybrid_with_aux_and_rectangular_sim(hip):
    """OrthLoss(weight, label_smoothing, dice_weight 0.5)(preds, target, proto_sim [4, 11], aux_preds): every entry of the dict equals the torch composition
    seg = ce + 0.5 dice, aux likewise, total = seg + 10 orth + 0.4 aux, dice_loss = the main head's unscaled Dice term (rtol 2e-5), and the gradients of both logit
    tensors follow (the kernel tolerances; the floor from the oracle's own fp32 error as in the kernel test)."""
    from segland_amd.loss.criterion import OrthLoss
    K, eps, lam, HW = 8, 0.1, 0.5, (64, 64)
    w = class_weights(K)
    preds, aux = fm.sym('dice/ol/preds', (2, K, 8, 8), 2.0), fm.sym('dice/ol/aux', (2, K, 16, 16), 1.5)
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='dice/ol/mask', block=8, ignore_rows=7)
    sim = fm.sym('dice/ol/sim', (4, 11), 1.0)

    def compose(dtype):
        pr, ar = preds.detach().to(dtype).clone().requires_grad_(True), aux.detach().to(dtype).clone().requires_grad_(True)
        up = lambda x: F.interpolate(x, size=HW, mode='bilinear', align_corners=True)
        ce = lambda u: F.cross_entropy(u, target, weight=w.to(dtype), ignore_index=255, label_smoothing=eps)
        upm, upa = up(pr), up(ar)
        dice = torch_dice(upm, target, w, 1.0)
        seg, auxl = ce(upm) + lam * dice, ce(upa) + lam * torch_dice(upa, target, w, 1.0)
        s = sim.to(dtype)
        orth = s[torch.triu(torch.ones_like(s), diagonal=1) == 1].abs().mean()
        ref = {'seg_loss': seg, 'aux_loss': auxl, 'orth_loss': orth, 'dice_loss': dice, 'total_loss': seg + orth * 10.0 + 0.4 * auxl}
        ref['total_loss'].backward()
        return ref, pr.grad.numpy(), ar.grad.numpy()

    ref, gp, ga = compose(torch.float32)
    _, gp64, ga64 = compose(torch.float64)
    crit = OrthLoss(255, weight=w, label_smoothing=eps, dice_weight=lam).to(DEV)
    assert crit.weight.is_cuda and len(crit.state_dict()) == 0
    pg, ag = preds.to(DEV).requires_grad_(True), aux.to(DEV).requires_grad_(True)
    d = crit(pg, target.to(DEV), is_ft=True, proto_sim=sim.to(DEV), aux_preds=ag)
    assert sorted(d) == sorted(ref)
    d['total_loss'].backward()
    for k in ref:
        print('%s: %.8g (torch %.8g)' % (k, float(d[k].detach()), float(ref[k].detach())))
        np.testing.assert_allclose(float(d[k].detach()), float(ref[k].detach()), rtol=2e-5, err_msg=k)
    valid = target[target != 255]
    floor = 2e-8 * float(w.max()) * valid.numel() / float(w.double()[valid].sum())
    for name, got, want, want64 in (('preds', pg.grad, gp, gp64), ('aux_preds', ag.grad, ga, ga64)):
        atol = max(floor, 8.0 * float(np.abs(want - want64).max()))
        print('   d total / d %s: max abs error %.3g, floor %.3g (max |grad| %.3g)' % (name, float(np.abs(got.cpu().numpy() - want).max()), atol, float(np.abs(want).max())))
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-3, atol=atol)
    # without aux_preds: no aux_loss, the add-with-alpha total
    d2 = crit(pg.detach(), target.to(DEV), proto_sim=sim.to(DEV))
    assert sorted(d2) == ['dice_loss', 'orth_loss', 'seg_loss', 'total_loss']
    np.testing.assert_allclose(float(d2['total_loss']), float(ref['seg_loss'].detach() + 10.0 * ref['orth_loss'].detach()), rtol=2e-5)
    assert torch.equal(d2['dice_loss'], d['dice_loss'].detach())


def test_reduce_loss_dict_carries_the_extra_key(hip):
    """engine.reduce_loss_dict and the drivers' log line iterate the dict: the Dice entry comes through as a float under its key"""
    from segland_amd.engine import Engine
    from segland_amd.loss.criterion import OrthLoss
    preds = fm.sym('dice/ol/preds', (2, 8, 8, 8), 2.0).to(DEV)
    target = fm.formula_mask(2, 64, 64, 8, tag='dice/ol/mask', block=8, ignore_rows=7).to(DEV)
    d = OrthLoss(255, dice_weight=0.5).to(DEV)(preds, target, proto_sim=fm.sym('dice/ol/sim', (4, 11), 1.0).to(DEV))
    eng = Engine.__new__(Engine)
    eng.distributed = False
    eng.world_size = 1
    vals = eng.reduce_loss_dict(d)
    assert list(vals) == list(d) and 'dice_loss' in vals
    for k in d:
        assert float(vals[k]) == float(d[k]), k
    line = ''.join(' %s=%.4f' % kv for kv in vals.items())
    assert ' dice_loss=%.4f' % float(d['dice_loss']) in line


# --------------------------------------------------------------------------------------------- 3. models
def _model(crit, **kw):
    from segland_amd.networks.pspnet_pop import GFSS_Model
    m = GFSS_Model(criterion=crit, backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=torch.float32, **kw)
    return fm.load_formula_weights(m).to(DEV)


def _torch_seg(logits, mask, w, eps, lam):
    up = F.interpolate(logits, size=tuple(mask.shape[1:]), mode='bilinear', align_corners=True)
    dice = torch_dice(up, mask, w, 1.0)
    return float(F.cross_entropy(up, mask, weight=w, ignore_index=255, label_smoothing=eps) + lam * dice), float(dice)


def test_base_model_uses_the_hybrid_loss(hip):
    """GFSS_Model(n_base=7) in train_mode() (backbone and decoder frozen), fp32, 2 x 64 x 64: seg_loss and dice_loss equal torch on the logits of a criterion-less call
    of the same model (rtol 2e-5); base_emb.grad is finite, non-zero and not the Dice-off run's."""
    from segland_amd.loss.criterion import OrthLoss
    K, eps, lam = 8, 0.1, 0.5
    w = class_weights(K)
    m = _model(OrthLoss(255, weight=w, label_smoothing=eps, dice_weight=lam), n_base=7)
    assert m.criterion.weight.is_cuda and not any('criterion' in k for k in m.state_dict())
    m.train_mode()
    for part in (m.backbone, m.decoder):
        for p in part.parameters():
            p.requires_grad = False
    img = fm.formula_image(2, 64, 64, 'dice/img').to(DEV)
    mask = fm.formula_mask(2, 64, 64, K, 'dice/mask', block=8, ignore_rows=4)
    d = m(img, mask.to(DEV))
    assert 'dice_loss' in d
    d['total_loss'].backward()
    g_d = m.base_emb.grad.detach().clone()
    crit, m.criterion = m.criterion, None
    with torch.no_grad():
        logits = m(img).float().cpu()
    assert tuple(logits.shape) == (2, K, 8, 8)
    seg, dice = _torch_seg(logits, mask, w, eps, lam)
    print('base mode seg_loss %.8g (torch on the model\'s logits %.8g), dice_loss %.8g (torch %.8g)' % (float(d['seg_loss'].detach()), seg, float(d['dice_loss'].detach()), dice))
    np.testing.assert_allclose(float(d['seg_loss'].detach()), seg, rtol=2e-5)
    np.testing.assert_allclose(float(d['dice_loss'].detach()), dice, rtol=2e-5)
    m.criterion = OrthLoss(255, weight=w, label_smoothing=eps).to(DEV)          # Dice off
    m.base_emb.grad = None
    dp = m(img, mask.to(DEV))
    assert 'dice_loss' not in dp
    dp['total_loss'].backward()
    np.testing.assert_allclose(float(dp['seg_loss'].detach()), _torch_seg(logits, mask, w, eps, 0.0)[0], rtol=2e-5)
    assert bool(torch.isfinite(g_d).all()) and float(g_d.abs().max()) > 0 and not torch.equal(g_d, m.base_emb.grad)
    m.criterion = crit


def test_ft_model_uses_the_hybrid_loss(hip):
    """Fine-tune mode, 1 + 7 + 4 = 12 logit channels, one novel and one base tile (as test_weighted_ce_gpu.test_ft_model_uses_the_weighted_loss): a criterion-less
    forward_novel on a clone of mask_b yields the logits and the pseudo-labelled mask; the call with the hybrid criterion on a fresh clone must give torch's seg_loss and
    dice_loss on those logits and that mask (rtol 2e-5)."""
    from segland_amd.loss.criterion import OrthLoss
    K, eps, lam = 12, 0.1, 0.5
    w = class_weights(K)
    m = _model(None, n_base=7, is_ft=True, n_novel=4)
    m.init_cls_n()
    m.train_mode()
    img, img_b = fm.formula_image(1, 64, 64, 'dice/ftimg').to(DEV), fm.formula_image(1, 64, 64, 'dice/ftimg_b').to(DEV)
    mask = fm.formula_mask(1, 64, 64, 4, 'dice/ftmask', block=8, ignore_rows=4) + 8
    mask[mask > 11] = 255                                                        # novel ids 8..11
    mask_b = fm.formula_mask(1, 64, 64, 8, 'dice/ftmask_b', block=8, ignore_rows=0)   # background + 7 base classes
    mb = mask_b.clone().to(DEV)
    with torch.no_grad():
        logits = m(img, mask.to(DEV), img_b, mb).float().cpu()
    assert tuple(logits.shape) == (2, K, 8, 8)
    mask_all = torch.cat([mask, mb.cpu()], 0)
    assert int((mb.cpu() != mask_b).sum()) > 0, 'no pseudo-label was written: the case checks less than it says'
    seg, dice = _torch_seg(logits, mask_all, w, eps, lam)
    m.criterion = OrthLoss(255, weight=w, label_smoothing=eps, dice_weight=lam).to(DEV)
    mb2 = mask_b.clone().to(DEV)
    d = m(img, mask.to(DEV), img_b, mb2)
    assert torch.equal(mb2, mb)
    print('fine-tune mode seg_loss %.8g (torch on the model\'s logits and pseudo-labels %.8g), dice_loss %.8g (torch %.8g)'
          % (float(d['seg_loss'].detach()), seg, float(d['dice_loss'].detach()), dice))
    np.testing.assert_allclose(float(d['seg_loss'].detach()), seg, rtol=2e-5)
    np.testing.assert_allclose(float(d['dice_loss'].detach()), dice, rtol=2e-5)
    d['total_loss'].backward()
    assert bool(torch.isfinite(m.novel_emb.grad).all()) and float(m.novel_emb.grad.abs().max()) > 0


# --------------------------------------------------------------------------------------------- 4. captured step
def test_captured_step_with_hybrid_loss_equals_eager(hip):
    """graph_step.GraphedTrainStep on PSPNet-POP fp32 (2 x 96 x 128, four batches, six steps) with Dice weight 0.5 and class weights against the same steps issued kernel
    by kernel, compared as test_graph_step_gpu.test_graphed_step_equals_eager compares them (losses, gradient norms, parameters: bit for bit); the last two steps are
    replays of one graph."""
    from segland_amd import graph_step
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    batches = [(fm.formula_image(2, 96, 128, 'dice/gs/img%d' % k).to(DEV), fm.formula_mask(2, 96, 128, 8, 'dice/gs/mask%d' % k, block=16, ignore_rows=4).to(DEV))
               for k in range(4)]
    ref = _model(OrthLoss(255, weight=class_weights(8), dice_weight=0.5), n_base=7).train()
    got = copy.deepcopy(ref)

    def run(model, graphed):
        opt = AdamW(get_parameters(model, lr=1e-4), lr=1e-4, weight_decay=1e-4)
        scaler = NativeScalerWithGradNormCount()
        step = graph_step.GraphedTrainStep(train_iteration, model, opt, scaler, double_step=True, warmup=2) if graphed else None
        log, graph_before = [], None
        for k in range(6):
            img, mask = batches[k % 4]
            if k == 5:
                graph_before = step.graph if graphed else None
            d, gn = step(img, mask) if graphed else train_iteration(model, opt, scaler, img, mask, double_step=True)
            assert 'dice_loss' in d
            log.append((float(d['total_loss'].detach()), float(d['seg_loss'].detach()), float(d['dice_loss'].detach()), float(gn)))
        if graphed:
            assert step.graph is not None and step.graph is graph_before and step.replays >= 2 and step.failures == 0, 'the last two steps were not replays of one graph'
        return log, {k: v.detach().float().cpu() for k, v in model.state_dict().items()}

    log_r, sd_r = run(ref, False)
    log_g, sd_g = run(got, True)
    print('losses / dice / grad norms eager vs graph:', log_r, log_g)
    assert log_r == log_g
    assert all(np.isfinite(v) for row in log_r for v in row) and all(row[2] > 0 for row in log_r)
    for k in sd_r:
        assert torch.equal(sd_r[k], sd_g[k]), k
