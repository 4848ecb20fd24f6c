"""Focal modulation in the fused upsample + loss kernels (csrc/loss.hip, sl_upsample_focal_fwd / _bwd and sl_upsample_focal_dice_fwd / _bwd) against the definition of
include/segland_hip.h in torch float64 (focal_reference.py; its float32 evaluation is the yardstick for the gradient's floor): every kernel route (forward, hybrid forward,
gather / tiled / channel-sliced tiled backward, both per-thread widths), saturated pixels, ignored samples, the hybrid and the mining composition, OrthLoss, the PSPNet-POP
model in base and fine-tune mode and a captured training step.  Without the focal entry points every test here fails (missing attribute / unexpected keyword)."""
import copy
import functools

import numpy as np
import pytest
import torch

import focal_reference as R
from oracle import formula as fm
from test_dice_loss_gpu import CE_CASES, MODES, class_weights, torch_dice

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GS = 0.7                         # upstream gradient
GAMMAS = [1.0, 2.0, 3.5]
# logit scale of the saturated cases (their shapes: CE_CASES[0] and [3]).  Chosen on the CPU with the float32 replay of the kernels' u (focal_reference.kernel_u): at
# 60 x the K = 8 map has pixels with u == 0 and pixels with 0 < u < 1; among 33 channels the runner-up is within exp's float32 range of the maximum almost everywhere
# at that scale (no pixel with u == 0), so that case takes 600 x.
SAT_SCALE = {8: 60.0, 33: 600.0}


@functools.lru_cache(maxsize=None)
def reference(K, hw, HW, weighted, eps, gamma, blank1=False, scale=1.0, lam=0.0, s=1.0):
    """loss, weight sum and d (GS * (loss + lam * dice)) / d logits in float64, and the floor of the gradient check: the larger of the weighted kernels' floor (2e-8 scaled
    by how far weighting can raise a pixel's share of the mean) and 8 x the float32 evaluation's own distance from float64 on the same gradient -- from the reference alone"""
    preds = fm.sym('focal/p%d' % K, (2, K) + hw, 3.0) * scale
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='focal/m%d' % K, block=8, ignore_rows=5)
    if blank1:
        target = torch.cat([target[:1], torch.full_like(target[1:], 255)])
    w = class_weights(K) if weighted else None
    extra = (lambda up: lam * torch_dice(up, target, w, s)) if lam else None
    loss32, _, g32 = R.focal_with_grad(preds, target, HW, gamma, w, eps, torch.float32, GS, extra)
    loss, wsum, g = R.focal_with_grad(preds, target, HW, gamma, w, eps, torch.float64, GS, extra)
    dice = float(torch_dice(R.upsample(preds.double(), HW), target, w, s)) if lam else None
    valid = target[target != 255]
    oracle_grad_err = float(np.abs(g32 - g).max())
    atol = max(2e-8 * (float(w.max()) if weighted else 1.0) * valid.numel() / wsum, 8.0 * oracle_grad_err)
    return dict(preds=preds, target=target, w=w, eps=eps, gamma=gamma, loss=loss, wsum=wsum, dice=dice, dref=g, atol=atol, lam=lam, s=s,
                oracle_loss_err=abs(loss32 - loss) / abs(loss), oracle_grad_err=oracle_grad_err)


def run_kernels(r):
    """forward + finalize and backward twice each: two runs must give the same bits.  -> (float [2] or [3] on the host, dlogits, coef or None)"""
    from segland_amd import ops
    pg, tg = r['preds'].to(DEV), r['target'].to(DEV)
    wg = None if r['w'] is None else r['w'].to(DEV)
    kw = dict(weight=wg, label_smoothing=r['eps'])
    if r['lam']:
        gs = torch.tensor([GS, GS * r['lam']], device=DEV)
        (out, coef), (out2, coef2) = (ops.upsample_focal_dice_fwd(pg, tg, 255, r['gamma'], smooth=r['s'], **kw) for _ in range(2))
        dl, dl2 = (ops.upsample_focal_dice_bwd(pg, tg, out, coef, gs, 255, r['gamma'], **kw) for _ in range(2))
        assert tuple(out.shape) == (3,) and torch.equal(coef, coef2)
    else:
        gs, coef = torch.tensor([GS], device=DEV), None
        out, out2 = (ops.upsample_focal_fwd(pg, tg, 255, r['gamma'], **kw) for _ in range(2))
        dl, dl2 = (ops.upsample_focal_bwd(pg, tg, out, gs, 255, r['gamma'], **kw) for _ in range(2))
        assert tuple(out.shape) == (2,)
    assert torch.equal(out, out2) and torch.equal(dl, dl2), 'run to run'
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dl).all())
    return out.cpu(), dl.cpu().numpy(), coef


def check_against(r, out, dl, what):
    print('%s: loss %.8g (float64 %.8g; torch fp32 is %.2g relative from it), weight sum %.8g (float64 %.8g)'
          % (what, out[0].item(), r['loss'], r['oracle_loss_err'], out[1].item(), r['wsum']))
    print('   gradient: max abs error %.3g, floor %.3g (max |grad| %.3g; torch fp32 is %.2g absolute from float64)'
          % (float(np.abs(dl - r['dref']).max()), r['atol'], float(np.abs(r['dref']).max()), r['oracle_grad_err']))
    np.testing.assert_allclose(out[0].item(), r['loss'], rtol=2e-5)
    np.testing.assert_allclose(out[1].item(), r['wsum'], rtol=2e-5)
    if r['lam']:
        print('   dice %.8g (float64 %.8g)' % (out[2].item(), r['dice']))
        np.testing.assert_allclose(out[2].item(), r['dice'], rtol=2e-5)
    np.testing.assert_allclose(dl, r['dref'], rtol=1e-3, atol=r['atol'])


# --------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_focal_kernels(hip, K, hw, HW, mode, route, gamma):
    """loss and weight sum rtol 2e-5 against float64 (the bound of these kernels); gradient of 0.7 * loss rtol 1e-3 with the reference's floor.  The two samples differ
    (rows 0..4 of sample 0 are ignored, the label maps are independent).  Both distances are printed beside each result."""
    weighted, eps = MODES[mode]
    r = reference(K, hw, HW, weighted, eps, gamma)
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl, _ = run_kernels(r)
    check_against(r, out, dl, 'K %d %s -> %s, %s, gamma %g, %s backward' % (K, hw, HW, mode, gamma, route))


# --------------------------------------------------------------------------------------------- 2. saturated pixels
@pytest.mark.parametrize('gamma', [1.0, 2.0])
@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('mode', ['plain', 'weights+smoothing'])
@pytest.mark.parametrize('K,hw,HW', [CE_CASES[0], CE_CASES[3]])
def test_saturated_pixels(hip, K, hw, HW, mode, route, gamma):
    """Logits scaled until, in the kernels' float32 arithmetic, some valid pixels have u == 0 exactly (every other exponential underflows: mod = beta = 0, no 0 * inf, no
    0^0) and others 0 < u < 1; asserted first, from the float32 replay.  Every output is finite (run_kernels) and within the bounds of the kernel test."""
    weighted, eps = MODES[mode]
    r = reference(K, hw, HW, weighted, eps, gamma, scale=SAT_SCALE[K])
    u = R.kernel_u(R.upsample(r['preds'], HW), r['target'])
    n0, nmid = int((u == 0).sum()), int(((u > 0) & (u < 1)).sum())
    print('K %d, logits x %g: %d of %d valid pixels with u == 0, %d with 0 < u < 1' % (K, SAT_SCALE[K], n0, u.size, nmid))
    assert n0 >= 1 and nmid >= 1
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl, _ = run_kernels(r)
    check_against(r, out, dl, 'K %d saturated, %s, gamma %g, %s backward' % (K, mode, gamma, route))


# --------------------------------------------------------------------------------------------- 3. ignored pixels
@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_a_fully_ignored_sample_has_a_zero_gradient(hip, K, hw, HW, route):
    weighted, eps = MODES['weights+smoothing']
    r = reference(K, hw, HW, weighted, eps, 2.0, blank1=True)
    assert not r['dref'][1].any()
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl, _ = run_kernels(r)
    check_against(r, out, dl, 'K %d %s -> %s, sample 1 ignored, %s backward' % (K, hw, HW, route))
    assert not dl[1].any(), 'gradient of a sample without a valid pixel'
    assert np.abs(dl[0]).max() > 0


def test_out_of_range_labels_count_as_ignored(hip):
    """labels outside [0, K) count as ignored: 250 (and a negative one) in the place of some labels gives the results of 255 there, bit for bit, in both pairs"""
    from segland_amd import ops
    r = reference(8, (8, 8), (64, 64), True, 0.1, 2.0)
    pg, wg = r['preds'].to(DEV), r['w'].to(DEV)
    t255 = r['target'].clone()
    t255[1, 10:20, 7:50] = 255
    t250 = t255.clone()
    t250[1, 10:20, 7:50] = 250
    t250[1, 12, 9] = -3
    res = []
    for t in (t255.to(DEV), t250.to(DEV)):
        out = ops.upsample_focal_fwd(pg, t, 255, 2.0, weight=wg, label_smoothing=0.1)
        dl = ops.upsample_focal_bwd(pg, t, out, torch.tensor([GS], device=DEV), 255, 2.0, weight=wg, label_smoothing=0.1)
        out3, coef = ops.upsample_focal_dice_fwd(pg, t, 255, 2.0, weight=wg, label_smoothing=0.1)
        dl3 = ops.upsample_focal_dice_bwd(pg, t, out3, coef, torch.tensor([GS, GS], device=DEV), 255, 2.0, weight=wg, label_smoothing=0.1)
        res.append((out, dl, out3, coef, dl3))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------- 4. hybrid
@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('K,hw,HW', [CE_CASES[0], CE_CASES[2]])
def test_hybrid_modulates_the_cross_entropy_part_only(hip, K, hw, HW, route):
    """gscale = (0.7, 0.7 * 0.25), smooth = 2.5, weights + smoothing 0.1, gamma 2: loss, weight sum, Dice and the gradient of 0.7 * (focal + 0.25 * dice) against float64;
    the Dice value and the coefficient table are bit-equal to what the hybrid pair without focal gives on the same inputs (the Dice sums do not see the modulation)."""
    from segland_amd import ops
    r = reference(K, hw, HW, True, 0.1, 2.0, lam=0.25, s=2.5)
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl, coef = run_kernels(r)
    check_against(r, out, dl, 'K %d %s -> %s, focal + 0.25 dice, smooth 2.5, %s backward' % (K, hw, HW, route))
    out0, coef0 = ops.upsample_ce_dice_fwd(r['preds'].to(DEV), r['target'].to(DEV), 255, weight=r['w'].to(DEV), label_smoothing=0.1, smooth=2.5)
    assert torch.equal(out0[2].cpu(), out[2]) and torch.equal(out0[1].cpu(), out[1]) and torch.equal(coef0, coef)
    assert not torch.equal(out0[0].cpu(), out[0])


# --------------------------------------------------------------------------------------------- 5. mining in front
@pytest.mark.parametrize('lam', [0.0, 0.5])
def test_mining_runs_in_front_on_the_unmodulated_probabilities(hip, lam):
    """OrthLoss(ohem_thresh 0.7, small ohem_min_kept, focal_gamma 2): loss and gradient equal, bit for bit, the focal ops run on the label map OrthLoss.mine returns"""
    from segland_amd import ops
    from segland_amd.loss.criterion import OrthLoss
    r = reference(8, (8, 8), (64, 64), True, 0.1, 2.0)
    crit = OrthLoss(255, weight=r['w'], label_smoothing=0.1, dice_weight=lam, ohem_thresh=0.7, ohem_min_kept=300, focal_gamma=2.0).to(DEV)
    pg, tg = r['preds'].to(DEV).requires_grad_(True), r['target'].to(DEV)
    mined, frac = crit.mine(pg, tg)
    assert 0.0 < float(frac) < 1.0 and not torch.equal(mined, tg)
    seg, dice, frac2 = crit.head_loss(pg, tg)
    (seg * GS).backward()
    assert torch.equal(frac, frac2)
    if lam:
        out, coef = ops.upsample_focal_dice_fwd(pg.detach(), mined, 255, 2.0, weight=crit.weight, label_smoothing=0.1, smooth=1.0)
        gs = torch.tensor([GS, GS * lam], device=DEV)
        want = ops.upsample_focal_dice_bwd(pg.detach(), mined, out, coef, gs, 255, 2.0, weight=crit.weight, label_smoothing=0.1)
        assert torch.equal(seg.detach(), torch.add(out[0], out[2], alpha=lam)) and torch.equal(dice.detach(), out[2])
    else:
        out = ops.upsample_focal_fwd(pg.detach(), mined, 255, 2.0, weight=crit.weight, label_smoothing=0.1)
        want = ops.upsample_focal_bwd(pg.detach(), mined, out, torch.tensor([GS], device=DEV), 255, 2.0, weight=crit.weight, label_smoothing=0.1)
        assert torch.equal(seg.detach(), out[0]) and dice is None
    assert torch.equal(pg.grad, want)


# --------------------------------------------------------------------------------------------- 6. OrthLoss
def test_orth_loss_focal_with_aux_and_rectangular_sim(hip):
    """OrthLoss(weight, label_smoothing, focal_gamma 2)(preds, target, proto_sim [4, 11], aux_preds): the keys of the criterion without focal, every entry equal to the
    float64 composition seg = focal(main), aux = focal(aux), total = seg + 10 orth + 0.4 aux (rtol 2e-5), and the gradients of both logit tensors within the kernel bounds"""
    from segland_amd.loss.criterion import OrthLoss
    K, eps, gamma, HW = 8, 0.1, 2.0, (64, 64)
    w = class_weights(K)
    preds, aux = fm.sym('focal/ol/preds', (2, K, 8, 8), 2.0), fm.sym('focal/ol/aux', (2, K, 16, 16), 1.5)
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='focal/ol/mask', block=8, ignore_rows=7)
    sim = fm.sym('focal/ol/sim', (4, 11), 1.0)

    def compose(dtype):
        pr, ar = preds.to(dtype).clone().requires_grad_(True), aux.to(dtype).clone().requires_grad_(True)
        seg, auxl = (R.focal_loss(R.upsample(x, HW), target, gamma, w, eps)[0] for x in (pr, ar))
        s = sim.to(dtype)
        orth = s[torch.triu(torch.ones_like(s), diagonal=1) == 1].abs().mean()
        ref = {'seg_loss': seg, 'aux_loss': auxl, 'orth_loss': orth, 'total_loss': seg + orth * 10.0 + 0.4 * auxl}
        ref['total_loss'].backward()
        return ref, pr.grad.numpy(), ar.grad.numpy()

    _, gp32, ga32 = compose(torch.float32)
    ref, gp, ga = compose(torch.float64)
    crit = OrthLoss(255, weight=w, label_smoothing=eps, focal_gamma=gamma).to(DEV)
    assert crit.weight.is_cuda and len(crit.state_dict()) == 0
    pg, ag = preds.to(DEV).requires_grad_(True), aux.to(DEV).requires_grad_(True)
    d = crit(pg, target.to(DEV), is_ft=True, proto_sim=sim.to(DEV), aux_preds=ag)
    assert list(d) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss']
    d['total_loss'].backward()
    for k in ref:
        print('%s: %.8g (float64 %.8g)' % (k, float(d[k].detach()), float(ref[k].detach())))
        np.testing.assert_allclose(float(d[k].detach()), float(ref[k].detach()), rtol=2e-5, err_msg=k)
    valid = target[target != 255]
    floor = 2e-8 * float(w.max()) * valid.numel() / float(w.double()[valid].sum())
    for name, got, want, want32 in (('preds', pg.grad, gp, gp32), ('aux_preds', ag.grad, ga, ga32)):
        atol = max(floor, 8.0 * float(np.abs(want32 - want).max()))
        print('   d total / d %s: max abs error %.3g, floor %.3g (max |grad| %.3g)' % (name, float(np.abs(got.cpu().numpy() - want).max()), atol, float(np.abs(want).max())))
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-3, atol=atol)


# --------------------------------------------------------------------------------------------- 7. models
def _model(crit, **kw):
    from segland_amd.networks.pspnet_pop import GFSS_Model
    m = GFSS_Model(criterion=crit, backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=torch.float32, **kw)
    return fm.load_formula_weights(m).to(DEV)


@pytest.fixture
def focal_calls(monkeypatch):
    """names of the focal ops in call order; the ops still run"""
    from segland_amd import ops
    seen = []
    for name in ('upsample_focal_fwd', 'upsample_focal_bwd', 'upsample_focal_dice_fwd', 'upsample_focal_dice_bwd'):
        def wrap(*a, _f=getattr(ops, name), _n=name, **kw):
            seen.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, wrap)
    return seen


def _focal_of(logits, mask, w, eps, gamma):
    return float(R.focal_loss(R.upsample(logits.double(), tuple(mask.shape[1:])), mask, gamma, w, eps)[0])


def test_base_model_uses_the_focal_loss(hip, focal_calls):
    """GFSS_Model(n_base=7) in train_mode() (backbone and decoder frozen), fp32, 2 x 64 x 64, focal_gamma 2: the step reaches the focal pair, seg_loss equals the float64
    definition on the logits of a criterion-less call of the same model (rtol 2e-5); base_emb.grad is finite and non-zero"""
    from segland_amd.loss.criterion import OrthLoss
    K, eps, gamma = 8, 0.1, 2.0
    w = class_weights(K)
    m = _model(OrthLoss(255, weight=w, label_smoothing=eps, focal_gamma=gamma), n_base=7)
    assert not any('criterion' in k for k in m.state_dict())
    m.train_mode()
    for part in (m.backbone, m.decoder):
        for p in part.parameters():
            p.requires_grad = False
    img = fm.formula_image(2, 64, 64, 'focal/img').to(DEV)
    mask = fm.formula_mask(2, 64, 64, K, 'focal/mask', block=8, ignore_rows=4)
    d = m(img, mask.to(DEV))
    d['total_loss'].backward()
    assert 'upsample_focal_fwd' in focal_calls and 'upsample_focal_bwd' in focal_calls
    crit, m.criterion = m.criterion, None
    with torch.no_grad():
        logits = m(img).float().cpu()
    m.criterion = crit
    want = _focal_of(logits, mask, w, eps, gamma)
    print('base mode seg_loss %.8g (float64 definition on the model\'s logits %.8g)' % (float(d['seg_loss'].detach()), want))
    np.testing.assert_allclose(float(d['seg_loss'].detach()), want, rtol=2e-5)
    g = m.base_emb.grad
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_ft_model_uses_the_focal_loss(hip, focal_calls):
    """Fine-tune mode, 1 + 7 + 4 = 12 logit channels, one novel and one base tile (as test_dice_loss_gpu.test_ft_model_uses_the_hybrid_loss): the call with the focal
    criterion reaches the focal pair and gives the float64 definition's seg_loss on the logits and the pseudo-labelled mask of a criterion-less call (rtol 2e-5)"""
    from segland_amd.loss.criterion import OrthLoss
    K, eps, gamma = 12, 0.1, 2.0
    w = class_weights(K)
    m = _model(None, n_base=7, is_ft=True, n_novel=4)
    m.init_cls_n()
    m.train_mode()
    img, img_b = fm.formula_image(1, 64, 64, 'focal/ftimg').to(DEV), fm.formula_image(1, 64, 64, 'focal/ftimg_b').to(DEV)
    mask = fm.formula_mask(1, 64, 64, 4, 'focal/ftmask', block=8, ignore_rows=4) + 8
    mask[mask > 11] = 255                                                        # novel ids 8..11
    mask_b = fm.formula_mask(1, 64, 64, 8, 'focal/ftmask_b', block=8, ignore_rows=0)   # background + 7 base classes
    mb = mask_b.clone().to(DEV)
    with torch.no_grad():
        logits = m(img, mask.to(DEV), img_b, mb).float().cpu()
    assert tuple(logits.shape) == (2, K, 8, 8)
    want = _focal_of(logits, torch.cat([mask, mb.cpu()], 0), w, eps, gamma)
    m.criterion = OrthLoss(255, weight=w, label_smoothing=eps, focal_gamma=gamma).to(DEV)
    mb2 = mask_b.clone().to(DEV)
    d = m(img, mask.to(DEV), img_b, mb2)
    assert torch.equal(mb2, mb)
    d['total_loss'].backward()
    assert 'upsample_focal_fwd' in focal_calls and 'upsample_focal_bwd' in focal_calls
    print('fine-tune mode seg_loss %.8g (float64 definition on the model\'s logits and pseudo-labels %.8g)' % (float(d['seg_loss'].detach()), want))
    np.testing.assert_allclose(float(d['seg_loss'].detach()), want, rtol=2e-5)
    assert bool(torch.isfinite(m.novel_emb.grad).all()) and float(m.novel_emb.grad.abs().max()) > 0


def test_captured_step_with_focal_loss_equals_eager(hip):
    """graph_step.GraphedTrainStep on PSPNet-POP fp32 (2 x 96 x 128, four batches, six steps) with focal_gamma 2, class weights and Dice weight 0.5 against the same steps
    issued kernel by kernel (losses, gradient norms, parameters: bit for bit, as test_dice_loss_gpu.test_captured_step_with_hybrid_loss_equals_eager compares them); the
    last two steps are replays of one graph.  gamma is a kernel argument: the capture bakes it in."""
    from segland_amd import graph_step
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    batches = [(fm.formula_image(2, 96, 128, 'focal/gs/img%d' % k).to(DEV), fm.formula_mask(2, 96, 128, 8, 'focal/gs/mask%d' % k, block=16, ignore_rows=4).to(DEV))
               for k in range(4)]
    ref = _model(OrthLoss(255, weight=class_weights(8), dice_weight=0.5, focal_gamma=2.0), n_base=7).train()
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
            log.append((float(d['total_loss'].detach()), float(d['seg_loss'].detach()), float(d['dice_loss'].detach()), float(gn)))
        if graphed:
            assert step.graph is not None and step.graph is graph_before and step.replays >= 2 and step.failures == 0, 'the last two steps were not replays of one graph'
        return log, {k: v.detach().float().cpu() for k, v in model.state_dict().items()}

    log_r, sd_r = run(ref, False)
    log_g, sd_g = run(got, True)
    print('losses / dice / grad norms eager vs graph:', log_r, log_g)
    assert log_r == log_g
    assert all(np.isfinite(v) for row in log_r for v in row)
    for k in sd_r:
        assert torch.equal(sd_r[k], sd_g[k]), k
