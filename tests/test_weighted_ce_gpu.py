"""Class weights and label smoothing in the fused upsample + cross-entropy kernels (csrc/loss.hip, sl_upsample_ce_weighted_fwd / _bwd) against
torch.nn.functional.cross_entropy(F.interpolate(..., align_corners=True), weight, ignore_index, label_smoothing) evaluated in fp32 on the CPU of this machine: every
kernel (forward, gather / tiled / channel-sliced tiled backward, both per-thread widths), the plain path, OrthLoss, the PSPNet-POP model in base and fine-tune mode,
and a captured training step that follows an in-place update of the weights.  Without the weighted entry points every test here fails (TypeError / missing symbol)."""
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
# both per-thread widths (16, 33), one / two / three channel slices of the wide tiled backward, a ragged map, the identity scale
CE_CASES = [(8, (8, 8), (64, 64)), (12, (9, 7), (40, 33)), (21, (9, 7), (40, 33)), (33, (8, 8), (64, 64)), (33, (8, 8), (8, 8))]
MODES = {'weights': (True, 0.0), 'smoothing': (False, 0.1), 'weights+smoothing': (True, 0.1)}


def class_weights(K):
    """[0.5, 2] with one class (one that occurs in every label map used here but the single-block 8 x 8 one) at 0"""
    w = 1.25 + fm.sym('wce/w%d' % K, (K,), 0.75)
    w[K // 2] = 0.0
    return w


def torch_ce(preds, target, HW, w, eps, dtype):
    """(loss, d (GS * loss) / d preds) of the oracle expression in `dtype`"""
    pr = preds.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(F.interpolate(pr, size=HW, mode='bilinear', align_corners=True), target, weight=None if w is None else w.to(dtype), ignore_index=255,
                           reduction='mean', label_smoothing=eps)
    (loss * GS).backward()
    return float(loss.detach()), pr.grad.numpy()


@functools.lru_cache(maxsize=None)
def ce_reference(K, hw, HW, weighted, eps):
    preds = fm.sym('wce/p%d' % K, (2, K) + hw, 3.0)
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='wce/m%d' % K, block=8, ignore_rows=5)
    w = class_weights(K) if weighted else None
    ref, dref = torch_ce(preds, target, HW, w, eps, torch.float32)
    ref64, dref64 = torch_ce(preds, target, HW, w, eps, torch.float64)
    valid = target[target != 255]
    wsum = float((w.double()[valid]).sum()) if weighted else float(valid.numel())
    # the plain floor 2e-8 scaled by how far weighting can raise a pixel's share of the mean: max(w) / (sum_p w_t / n_valid)
    atol = 2e-8 * (float(w.max()) if weighted else 1.0) * valid.numel() / wsum
    return dict(preds=preds, target=target, w=w, ref=ref, dref=dref, wsum=wsum, atol=atol,
                oracle_loss_err=abs(ref - ref64) / abs(ref64), oracle_grad_err=float(np.abs(dref - dref64).max()))


def run_kernels(r, eps, weight='own'):
    from segland_amd import ops
    pg, tg = r['preds'].to(DEV), r['target'].to(DEV)
    wg = (None if r['w'] is None else r['w'].to(DEV)) if isinstance(weight, str) else weight
    gs = torch.full((1,), GS, device=DEV)
    out = ops.upsample_ce_fwd(pg, tg, 255, weight=wg, label_smoothing=eps)
    out2 = ops.upsample_ce_fwd(pg, tg, 255, weight=wg, label_smoothing=eps)
    dl = ops.upsample_ce_bwd(pg, tg, out, gs, 255, weight=wg, label_smoothing=eps)
    dl2 = ops.upsample_ce_bwd(pg, tg, out, gs, 255, weight=wg, label_smoothing=eps)
    assert torch.equal(out, out2) and torch.equal(dl, dl2), 'run to run'
    assert bool(torch.isfinite(dl).all())
    return out.cpu(), dl.cpu().numpy()


def check_against(r, out, dl, what):
    print('%s: loss %.8g (torch %.8g, torch fp32 is %.2g relative from float64), weight sum %.8g (float64 %.8g)'
          % (what, out[0].item(), r['ref'], r['oracle_loss_err'], out[1].item(), r['wsum']))
    print('   gradient: max abs error %.3g, floor %.3g (max |grad| %.3g; torch fp32 is %.2g absolute from float64)'
          % (float(np.abs(dl - r['dref']).max()), r['atol'], float(np.abs(r['dref']).max()), r['oracle_grad_err']))
    np.testing.assert_allclose(out[0].item(), r['ref'], rtol=2e-5)
    np.testing.assert_allclose(out[1].item(), r['wsum'], rtol=2e-5)
    np.testing.assert_allclose(dl, r['dref'], rtol=1e-3, atol=r['atol'])


# --------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_weighted_ce_kernels(hip, K, hw, HW, mode, route):
    """Loss rtol 2e-5, gradient rtol 1e-3 with the absolute floor 2e-8 * max(w) * n_valid / sum_p w_t, out[1] against the float64 weight sum rtol 2e-5 (the bounds of
    test_wide_head_gpu.test_upsample_ce_wide; the floor scaled by how far weighting can raise one pixel's share of the mean).  The oracle's own distance from a float64
    evaluation of the same expression is printed beside each result."""
    weighted, eps = MODES[mode]
    r = ce_reference(K, hw, HW, weighted, eps)
    assert HW == (8, 8) or len(r['target'].unique()) == K + 1         # every class occurs, the zero-weight one too (an 8 x 8 label map has one block)
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl = run_kernels(r, eps)
    check_against(r, out, dl, 'K %d %s -> %s, %s, %s backward' % (K, hw, HW, mode, route))


# --------------------------------------------------------------------------------------------- 2. the plain path
@pytest.mark.parametrize('K,hw,HW', [CE_CASES[0], CE_CASES[3]])
def test_plain_path_and_unit_weights(hip, K, hw, HW):
    """ops.upsample_ce_fwd / bwd with their defaults (the plain kernels) meet the unweighted oracle, and so do the weighted kernels with weights of one and no
    smoothing, on both backward routes; out[1] of the plain path is the exact pixel count."""
    r = ce_reference(K, hw, HW, False, 0.0)
    ones = torch.ones(K, device=DEV)
    for route in ('tiled', 'gather'):
        hip.sl_debug_ce_tiled(1 if route == 'tiled' else 0)
        out, dl = run_kernels(r, 0.0)
        check_against(r, out, dl, 'K %d plain, %s' % (K, route))
        assert out[1].item() == float((r['target'] != 255).sum())
        out1, dl1 = run_kernels(r, 0.0, weight=ones)
        check_against(r, out1, dl1, 'K %d unit weights through the weighted kernels, %s' % (K, route))
        print('   unit weights vs plain: loss %s, gradient %s' % ('bit-equal' if torch.equal(out, out1) else 'differs', 'bit-equal' if np.array_equal(dl, dl1) else 'differs'))


def test_ops_refuse_a_wrong_weight_vector(hip):
    from segland_amd import ops
    r = ce_reference(8, (8, 8), (64, 64), False, 0.0)
    pg, tg = r['preds'].to(DEV), r['target'].to(DEV)
    with pytest.raises(ValueError, match='7 class weights for 8 logit channels'):
        ops.upsample_ce_fwd(pg, tg, 255, weight=torch.ones(7, device=DEV))
    with pytest.raises(ValueError):
        ops.upsample_ce_fwd(pg, tg, 255, weight=torch.ones(8))                      # on the CPU
    with pytest.raises(ValueError):
        ops.upsample_ce_fwd(pg, tg, 255, weight=torch.ones(8, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='label_smoothing'):
        ops.upsample_ce_fwd(pg, tg, 255, label_smoothing=1.5)


# --------------------------------------------------------------------------------------------- 3. OrthLoss
def test_orth_loss_weighted_with_aux_and_rectangular_sim(hip):
    """OrthLoss(weight, label_smoothing)(preds, target, proto_sim [4, 11], aux_preds): every entry of the dict equals the torch composition seg + 10 orth + 0.4 aux with
    the weighted, smoothed cross-entropy in both places (rtol 2e-5), and the gradients of both logit tensors follow (the kernel tolerances)."""
    from segland_amd.loss.criterion import OrthLoss
    K, eps, HW = 8, 0.1, (64, 64)
    w = class_weights(K)
    preds, aux = fm.sym('wce/ol/preds', (2, K, 8, 8), 2.0), fm.sym('wce/ol/aux', (2, K, 16, 16), 1.5)
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='wce/ol/mask', block=8, ignore_rows=7)
    sim = fm.sym('wce/ol/sim', (4, 11), 1.0)
    # torch composition (criterion.py:37-43, 56-60)
    pr, ar = preds.clone().requires_grad_(True), aux.clone().requires_grad_(True)
    ce = lambda x: F.cross_entropy(F.interpolate(x, size=HW, mode='bilinear', align_corners=True), target, weight=w, ignore_index=255, label_smoothing=eps)
    seg, auxl = ce(pr), ce(ar)
    orth = sim[torch.triu(torch.ones_like(sim), diagonal=1) == 1].abs().mean()
    ref = {'seg_loss': seg, 'aux_loss': auxl, 'orth_loss': orth, 'total_loss': seg + orth * 10.0 + 0.4 * auxl}
    ref['total_loss'].backward()
    crit = OrthLoss(255, weight=w, label_smoothing=eps).to(DEV)
    assert crit.weight.is_cuda and len(crit.state_dict()) == 0
    pg, ag = preds.to(DEV).requires_grad_(True), aux.to(DEV).requires_grad_(True)
    d = crit(pg, target.to(DEV), is_ft=True, proto_sim=sim.to(DEV), aux_preds=ag)
    assert sorted(d) == sorted(ref)
    d['total_loss'].backward()
    for k in ref:
        print('%s: %.8g (torch %.8g)' % (k, float(d[k].detach()), float(ref[k].detach())))
        np.testing.assert_allclose(float(d[k].detach()), float(ref[k].detach()), rtol=2e-5, err_msg=k)
    valid = target[target != 255]
    atol = 2e-8 * float(w.max()) * valid.numel() / float(w.double()[valid].sum())
    np.testing.assert_allclose(pg.grad.cpu().numpy(), pr.grad.numpy(), rtol=1e-3, atol=atol)
    np.testing.assert_allclose(ag.grad.cpu().numpy(), ar.grad.numpy(), rtol=1e-3, atol=atol)
    with pytest.raises(ValueError, match='7 class weights for 8 logit channels'):
        OrthLoss(255, weight=w[:7]).to(DEV)(pg, target.to(DEV), proto_sim=sim.to(DEV))


# --------------------------------------------------------------------------------------------- 4. models
def _model(crit, **kw):
    from segland_amd.networks.pspnet_pop import GFSS_Model
    m = GFSS_Model(criterion=crit, backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=torch.float32, **kw)
    return fm.load_formula_weights(m).to(DEV)


def test_base_model_uses_the_weighted_loss(hip):
    """GFSS_Model(n_base=7) with BatchNorm on its running statistics (train_mode(); backbone and decoder frozen, as in fine-tuning): model(img, mask)['seg_loss'] equals
    torch's weighted, smoothed loss on the logits of a criterion-less call of the same model (rtol 2e-5); base_emb.grad is finite and not the unweighted run's."""
    from segland_amd.loss.criterion import OrthLoss
    K, eps = 8, 0.1
    w = class_weights(K)
    m = _model(OrthLoss(255, weight=w, label_smoothing=eps), n_base=7)
    assert m.criterion.weight.is_cuda and not any('criterion' in k for k in m.state_dict())      # moved with the model, and no key of its own
    m.train_mode()
    for part in (m.backbone, m.decoder):
        for p in part.parameters():
            p.requires_grad = False
    img = fm.formula_image(2, 64, 64, 'wce/img').to(DEV)
    mask = fm.formula_mask(2, 64, 64, K, 'wce/mask', block=8, ignore_rows=4)
    d = m(img, mask.to(DEV))
    d['total_loss'].backward()
    g_w = m.base_emb.grad.detach().clone()
    crit, m.criterion = m.criterion, None
    with torch.no_grad():
        logits = m(img).float().cpu()
    assert tuple(logits.shape) == (2, K, 8, 8)
    ref = F.cross_entropy(F.interpolate(logits, size=(64, 64), mode='bilinear', align_corners=True), mask, weight=w, ignore_index=255, label_smoothing=eps)
    print('base mode seg_loss %.8g (torch on the model\'s logits %.8g)' % (float(d['seg_loss'].detach()), float(ref)))
    np.testing.assert_allclose(float(d['seg_loss'].detach()), float(ref), rtol=2e-5)
    m.criterion = OrthLoss(255).to(DEV)
    m.base_emb.grad = None
    dp = m(img, mask.to(DEV))
    dp['total_loss'].backward()
    plain = F.cross_entropy(F.interpolate(logits, size=(64, 64), mode='bilinear', align_corners=True), mask, ignore_index=255)
    np.testing.assert_allclose(float(dp['seg_loss'].detach()), float(plain), rtol=2e-5)
    assert bool(torch.isfinite(g_w).all()) and float(g_w.abs().max()) > 0 and not torch.equal(g_w, m.base_emb.grad)
    m.criterion = crit


def test_ft_model_uses_the_weighted_loss(hip):
    """Fine-tune mode, 1 + 7 + 4 = 12 logit channels, one novel and one base tile: a criterion-less forward_novel on a clone of mask_b yields the logits and the
    pseudo-labelled mask; the call with the weighted criterion on a fresh clone must give torch's loss on those logits and that mask (rtol 2e-5).  Eleven weights
    (the channel count of another mode) are refused with both numbers."""
    from segland_amd.loss.criterion import OrthLoss
    K, eps = 12, 0.1
    w = class_weights(K)
    m = _model(None, n_base=7, is_ft=True, n_novel=4)
    m.init_cls_n()
    m.train_mode()
    img, img_b = fm.formula_image(1, 64, 64, 'wce/ftimg').to(DEV), fm.formula_image(1, 64, 64, 'wce/ftimg_b').to(DEV)
    mask = fm.formula_mask(1, 64, 64, 4, 'wce/ftmask', block=8, ignore_rows=4) + 8
    mask[mask > 11] = 255                                                        # novel ids 8..11
    mask_b = fm.formula_mask(1, 64, 64, 8, 'wce/ftmask_b', block=8, ignore_rows=0)   # background + 7 base classes
    mb = mask_b.clone().to(DEV)
    with torch.no_grad():
        logits = m(img, mask.to(DEV), img_b, mb).float().cpu()
    assert tuple(logits.shape) == (2, K, 8, 8)
    mask_all = torch.cat([mask, mb.cpu()], 0)
    assert int((mb.cpu() != mask_b).sum()) > 0, 'no pseudo-label was written: the case checks less than it says'
    ref = F.cross_entropy(F.interpolate(logits, size=(64, 64), mode='bilinear', align_corners=True), mask_all, weight=w, ignore_index=255, label_smoothing=eps)
    m.criterion = OrthLoss(255, weight=w, label_smoothing=eps).to(DEV)
    mb2 = mask_b.clone().to(DEV)
    d = m(img, mask.to(DEV), img_b, mb2)
    assert torch.equal(mb2, mb)
    print('fine-tune mode seg_loss %.8g (torch on the model\'s logits and pseudo-labels %.8g)' % (float(d['seg_loss'].detach()), float(ref)))
    np.testing.assert_allclose(float(d['seg_loss'].detach()), float(ref), rtol=2e-5)
    d['total_loss'].backward()
    assert bool(torch.isfinite(m.novel_emb.grad).all()) and float(m.novel_emb.grad.abs().max()) > 0
    m.criterion = OrthLoss(255, weight=w[:11]).to(DEV)
    with pytest.raises(ValueError, match='11 class weights for 12 logit channels'):
        m(img, mask.to(DEV), img_b, mask_b.clone().to(DEV))


# --------------------------------------------------------------------------------------------- 5. captured step
def _pspnet_weighted():
    from segland_amd.loss.criterion import OrthLoss
    return _model(OrthLoss(255, weight=class_weights(8), label_smoothing=0.1), n_base=7).train()


def _batches(n, B, H, W):
    return [(fm.formula_image(B, H, W, 'wce/gs/img%d' % k).to(DEV), fm.formula_mask(B, H, W, 8, 'wce/gs/mask%d' % k, block=16, ignore_rows=4).to(DEV)) for k in range(n)]


NEW_W = [2.0, 0.5, 0.0, 1.0, 1.5, 0.75, 1.25, 0.6]


def test_captured_step_with_weighted_loss_equals_eager(hip):
    """graph_step.GraphedTrainStep on PSPNet-POP fp32 (2 x 96 x 128, four batches, six steps) with the weighted, smoothed criterion against the same steps issued
    kernel by kernel, compared as test_graph_step_gpu.test_graphed_step_equals_eager compares them (losses, gradient norms, parameters: bit for bit).  Before the last
    step the class weights are overwritten in place on both sides: the replay reads the same device buffer, so it follows without a new capture."""
    from segland_amd import graph_step
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    batches = _batches(4, 2, 96, 128)
    ref = _pspnet_weighted()
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
                with torch.no_grad():
                    model.criterion.weight.copy_(torch.tensor(NEW_W))
            d, gn = step(img, mask) if graphed else train_iteration(model, opt, scaler, img, mask, double_step=True)
            log.append((float(d['total_loss'].detach()), float(d['seg_loss'].detach()), float(gn)))
        if graphed:
            assert step.graph is not None and step.graph is graph_before and step.replays >= 2 and step.failures == 0, 'the last two steps were not replays of one graph'
        return log, {k: v.detach().float().cpu() for k, v in model.state_dict().items()}

    log_r, sd_r = run(ref, False)
    log_g, sd_g = run(got, True)
    print('losses / grad norms eager vs graph:', log_r, log_g)
    assert log_r == log_g
    for k in sd_r:
        assert torch.equal(sd_r[k], sd_g[k]), k


def test_replay_follows_an_in_place_weight_update(hip):
    """With the learning rate at 0 a replay on the same batch repeats its loss bit for bit; after criterion.weight.copy_(...) the next replay of the SAME graph gives the
    loss of the new weights: torch's on the model's train-mode logits of that batch (rtol 2e-5), and not the old one."""
    from segland_amd import graph_step
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    m = _pspnet_weighted()
    opt = AdamW(get_parameters(m, lr=0.0), lr=0.0, weight_decay=0.0)
    step = graph_step.GraphedTrainStep(train_iteration, m, opt, NativeScalerWithGradNormCount(), warmup=2)
    img, mask = _batches(1, 2, 96, 128)[0]
    seg = [float(step(img, mask)[0]['seg_loss']) for _ in range(5)]
    graph, replays = step.graph, step.replays
    assert graph is not None and replays >= 2 and len(set(seg)) == 1, seg
    with torch.no_grad():
        m.criterion.weight.copy_(torch.tensor(NEW_W))
    after = float(step(img, mask)[0]['seg_loss'])
    assert step.graph is graph and step.replays == replays + 1 and step.failures == 0
    crit, m.criterion = m.criterion, None
    with torch.no_grad():
        logits = m(img).float().cpu()                    # train-mode BatchNorm: the batch statistics of this batch, as in the step
    m.criterion = crit
    up = F.interpolate(logits, size=(96, 128), mode='bilinear', align_corners=True)
    old = float(F.cross_entropy(up, mask.cpu(), weight=class_weights(8), ignore_index=255, label_smoothing=0.1))
    new = float(F.cross_entropy(up, mask.cpu(), weight=torch.tensor(NEW_W), ignore_index=255, label_smoothing=0.1))
    print('seg_loss before %.8g (torch %.8g), after the in-place update %.8g (torch %.8g)' % (seg[-1], old, after, new))
    np.testing.assert_allclose(seg[-1], old, rtol=2e-5)
    np.testing.assert_allclose(after, new, rtol=2e-5)
    assert abs(new - old) > 1e-3 * abs(old)
