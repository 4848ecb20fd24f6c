"""Lovasz-softmax term in the fused upsample + loss kernels (csrc/loss.hip: sl_upsample_lovasz_hist, sl_lovasz_scan, sl_upsample_lovasz_bwd) against the definition of
include/segland_hip.h in torch float64 (lovasz_reference.py): the integer histograms, the scan, every backward route (gather / tiled / channel-sliced tiled, both
per-thread widths) x {plain, weights, weights + smoothing} x {focal off, gamma 2} x {Dice off, on}, absent classes, ignored samples, saturated pixels, OrthLoss, the
PSPNet-POP model in base and fine-tune mode and a captured training step.  Without the Lovasz entry points every test here fails (missing attribute / unexpected keyword).

Tolerances.  The histogram may differ from the float64 one only where an error sits within the margin m (8 x float32-vs-float64 of e, from the reference) of a bin edge:
at most one move per such (pixel, class) pair, two counts each.  The scan is checked on the kernel's OWN histogram (rtol 2e-5, the loss kernels' standing bound).  The
backward with a table that is constant per class cannot depend on a bin: rtol 1e-3 with the focal tests' floor.  With the real table the per-element slack of the
reference (what the near-edge pixels can move) is added; test_lovasz_cpu.py asserts that this slack stays below 5 % of max |grad| on these inputs."""
import copy
import functools

import numpy as np
import pytest
import torch

import focal_reference as FR
import lovasz_reference as R
from oracle import formula as fm
from test_dice_loss_gpu import CE_CASES, MODES, class_weights, torch_dice
from test_focal_loss_gpu import SAT_SCALE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GS = 0.7                         # upstream gradient
LAM, MU = 0.25, 0.5              # Dice and Lovasz weights of the composed gradients
NB = R.NB


def lovasz_fwd(preds, target, want_hist=True):
    from segland_amd import ops
    return ops.upsample_lovasz_fwd(preds.to(DEV), target.to(DEV), 255, want_hist=want_hist)


# --------------------------------------------------------------------------------------------- 1. histogram
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_histogram(hip, K, hw, HW):
    """per class sum_j F = T_c and sum_j (F + Bk) = n_valid exactly; L1 distance to the float64 histogram <= 2 x the reference's near-edge pair count; two runs equal bits"""
    r = R.case(K, hw, HW)
    (out, table, hist), (out2, table2, hist2) = (lovasz_fwd(r['preds'], r['target']) for _ in range(2))
    assert hist.dtype == torch.int32 and tuple(hist.shape) == (K, NB, 2) and tuple(table.shape) == (K, NB) and tuple(out.shape) == (2,)
    assert torch.equal(hist, hist2) and torch.equal(table, table2) and torch.equal(out, out2), 'run to run'
    h = hist.cpu().long()
    assert h[:, :, 0].sum(1).tolist() == [int((r['target'] == c).sum()) for c in range(K)]
    assert h.sum((1, 2)).tolist() == [r['n_valid']] * K
    l1 = int((h - r['hist']).abs().sum())
    print('K %d %s -> %s: L1 distance to the float64 histogram %d (bound %d: %d near-edge pairs of %d, margin %.3g)' % (K, hw, HW, l1, 2 * r['near_edge'], r['near_edge'], r['pairs'], r['m']))
    assert l1 <= 2 * r['near_edge']


# --------------------------------------------------------------------------------------------- 2. scan
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_scan(hip, K, hw, HW):
    """from the kernel's own histogram through the reference scan in float64: out[0] and the table rtol 2e-5 (table atol 1e-12), out[1] == n_present, and the loss within
    1 / NB of the exactly sorted one (1 / (2 NB) of quantisation plus the float32 error of e, far below the other half by the Lipschitz bound)"""
    r = R.case(K, hw, HW)
    out, table, hist = lovasz_fwd(r['preds'], r['target'])
    loss, tab, n_present = R.scan(hist.cpu().long())
    out, table = out.cpu(), table.cpu().double().numpy()
    print('K %d %s -> %s: loss %.8g (float64 scan of the same histogram %.8g, sorted %.8g), n_present %g (%d), table max rel error %.3g'
          % (K, hw, HW, out[0].item(), loss, r['exact'], out[1].item(), n_present, float(np.abs(table - tab.numpy()).max() / tab.abs().max())))
    np.testing.assert_allclose(out[0].item(), loss, rtol=2e-5)
    np.testing.assert_allclose(table, tab.numpy(), rtol=2e-5, atol=1e-12)
    assert out[1].item() == n_present == r['n_present']
    assert abs(out[0].item() - r['exact']) <= 1.0 / NB
    assert not table[(hist.cpu().sum(2) == 0).numpy()].any()


# --------------------------------------------------------------------------------------------- 3. / 4. backward
def const_table(K, n_valid):
    """constant per class, different between classes, of the real table's order of magnitude"""
    return ((0.5 + torch.arange(K, dtype=torch.float64) / K) / n_valid)[:, None].expand(K, NB).contiguous()


@functools.lru_cache(maxsize=None)
def composed(K, hw, HW, mode, gamma, dice, blank1=False):
    """(cross-entropy or focal loss, weight sum, Dice or None) in float64 and a function table -> (d GS (ce + LAM dice + MU lovasz) / d logits in float64, floor): the floor
    is the focal tests', the larger of 2e-8 scaled by how far weighting can raise a pixel's share of the mean and 8 x the float32 evaluation's own distance from float64 on
    the same gradient (the float32 evaluation reads the table at the float64 bins: a bin flip is the slack's business, not the floor's)"""
    weighted, eps = MODES[mode]
    r = R.case(K, hw, HW, blank1)
    preds, target = r['preds'], r['target']
    w = class_weights(K) if weighted else None
    bins = R.bins_of(R.errors(R.upsample(preds, target), target)[0])

    def grad_for(table):
        def extra(up):
            t = MU * R.surrogate(up, target, table, bins)
            return t + LAM * torch_dice(up, target, w, 1.0) if dice else t
        loss32, _, g32 = FR.focal_with_grad(preds, target, HW, gamma, w, eps, torch.float32, GS, extra)
        loss, wsum, g = FR.focal_with_grad(preds, target, HW, gamma, w, eps, torch.float64, GS, extra)
        valid = target[target != 255]
        atol = max(2e-8 * (float(w.max()) if weighted else 1.0) * valid.numel() / wsum, 8.0 * float(np.abs(g32 - g).max()))
        return loss, wsum, g, atol
    dref = float(torch_dice(R.upsample(preds, target), target, w, 1.0)) if dice else None
    return r, w, eps, dref, grad_for


def run_backward(r, w, eps, gamma, dice, table):
    """the forward of the chosen cross-entropy / Dice form and the one backward launch, twice: two runs must give the same bits"""
    from segland_amd import ops
    pg, tg = r['preds'].to(DEV), r['target'].to(DEV)
    kw = dict(weight=None if w is None else w.to(DEV), label_smoothing=eps)
    coef = None
    if dice:
        out, coef = ops.upsample_focal_dice_fwd(pg, tg, 255, gamma, **kw) if gamma else ops.upsample_ce_dice_fwd(pg, tg, 255, **kw)
    else:
        out = ops.upsample_focal_fwd(pg, tg, 255, gamma, **kw) if gamma else ops.upsample_ce_fwd(pg, tg, 255, **kw)
    gs = torch.tensor([GS, GS * LAM, GS * MU], device=DEV)
    tab = table.to(device=DEV, dtype=torch.float32).contiguous()
    dl, dl2 = (ops.upsample_lovasz_bwd(pg, tg, out, coef, tab, gs, 255, gamma, **kw) for _ in range(2))
    assert torch.equal(dl, dl2), 'run to run'
    assert bool(torch.isfinite(dl).all())
    return out.cpu(), dl.cpu().numpy()


@pytest.mark.parametrize('dice', [False, True])
@pytest.mark.parametrize('gamma', [0.0, 2.0])
@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_backward_routes_with_a_table_constant_per_class(hip, K, hw, HW, mode, route, gamma, dice):
    """the bin cannot matter, so the slack is zero: gradient of 0.7 (ce + 0.25 dice + 0.5 lovasz) rtol 1e-3 with the focal tests' floor.  'tiled' is the one-pass tiled
    kernel up to 16 channels and the channel-sliced one above; the K = 33, 8 x 8 -> 8 x 8 case is the identity scale."""
    r, w, eps, _, grad_for = composed(K, hw, HW, mode, gamma, dice)
    table = const_table(K, r['n_valid'])
    loss, wsum, g, atol = grad_for(table)
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl = run_backward(r, w, eps, gamma, dice, table)
    lov_only = R.grad(r['preds'], r['target'], table).numpy() * GS * MU
    print('K %d %s -> %s, %s, gamma %g, dice %s, %s backward: max abs error %.3g, floor %.3g (max |grad| %.3g, of which the Lovasz term %.3g)'
          % (K, hw, HW, mode, gamma, dice, route, float(np.abs(dl - g).max()), atol, float(np.abs(g).max()), float(np.abs(lov_only).max())))
    np.testing.assert_allclose(out[0].item(), loss, rtol=2e-5)
    assert float(np.abs(lov_only).max()) > 100 * atol                  # the term is well above the floor: a kernel that left it out fails
    np.testing.assert_allclose(dl, g, rtol=1e-3, atol=atol)


@pytest.mark.parametrize('mode,gamma,dice', [('plain', 0.0, False), ('weights+smoothing', 2.0, True)])
@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_backward_with_the_real_table(hip, K, hw, HW, route, mode, gamma, dice):
    """the kernel's own table read back, the reference's bins: per element |error| <= 1e-3 |ref| + floor + slack(table); the worst error is printed beside the floor and
    the slack"""
    r, w, eps, _, grad_for = composed(K, hw, HW, mode, gamma, dice)
    _, table = lovasz_fwd(r['preds'], r['target'], want_hist=False)
    table = table.cpu().double()
    loss, wsum, g, atol = grad_for(table)
    slack = (R.slack(r['preds'], r['target'], table, r['m']) * GS * MU).numpy()
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    out, dl = run_backward(r, w, eps, gamma, dice, table)
    err = np.abs(dl - g)
    bound = 1e-3 * np.abs(g) + atol + slack
    i = np.unravel_index(np.argmax(err - bound), err.shape)
    print('K %d %s -> %s, %s, gamma %g, dice %s, %s backward: max abs error %.3g, floor %.3g, max slack %.3g (max |grad| %.3g); closest to its bound: error %.3g of %.3g'
          % (K, hw, HW, mode, gamma, dice, route, float(err.max()), atol, float(slack.max()), float(np.abs(g).max()), float(err[i]), float(bound[i])))
    assert (err <= bound).all()


# --------------------------------------------------------------------------------------------- 5. edge cases
def test_a_class_absent_from_the_batch_has_a_zero_row_and_is_not_counted(hip):
    K, hw, HW = CE_CASES[4]
    r = R.case(K, hw, HW)
    out, table, hist = lovasz_fwd(r['preds'], r['target'])
    absent = (hist[:, :, 0].sum(1) == 0).cpu()
    assert int((~absent).sum()) == 7 == int(out[1].item())
    assert not table.cpu()[absent].any() and bool((table.cpu()[~absent].abs().sum(1) > 0).all())


@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('K,hw,HW', [CE_CASES[0], CE_CASES[3]])
def test_a_fully_ignored_sample_has_a_zero_gradient(hip, K, hw, HW, route):
    r, w, eps, _, grad_for = composed(K, hw, HW, 'weights+smoothing', 2.0, True, blank1=True)
    out, table, hist = lovasz_fwd(r['preds'], r['target'])
    assert hist.cpu().long().sum((1, 2)).tolist() == [r['n_valid']] * K
    assert abs(out[0].item() - r['exact']) <= 1.0 / NB
    table = table.cpu().double()
    loss, wsum, g, atol = grad_for(table)
    assert not g[1].any()
    slack = (R.slack(r['preds'], r['target'], table, r['m']) * GS * MU).numpy()
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    _, dl = run_backward(r, w, eps, 2.0, True, table)
    assert not dl[1].any(), 'gradient of a sample without a valid pixel'
    assert (np.abs(dl - g) <= 1e-3 * np.abs(g) + atol + slack).all() and np.abs(dl[0]).max() > 0


@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('K,hw,HW', [CE_CASES[0], CE_CASES[3]])
def test_everything_ignored(hip, K, hw, HW, route):
    """no valid pixel: loss 0, no present class, a zero table, and the gradient of the Lovasz term exactly 0 (the cross-entropy's mean over nothing is not asked for:
    its upstream gradient is 0 here), all values finite"""
    from segland_amd import ops
    preds, target = R.inputs(K, hw, HW)
    pg, tg = preds.to(DEV), torch.full_like(target, 255).to(DEV)
    out, table, hist = ops.upsample_lovasz_fwd(pg, tg, 255, want_hist=True)
    assert out.tolist() == [0.0, 0.0] and not table.any() and not hist.any()
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    ce = ops.upsample_ce_fwd(pg, tg, 255)
    dl = ops.upsample_lovasz_bwd(pg, tg, ce, None, table, torch.tensor([0.0, 0.0, GS], device=DEV), 255)
    assert bool(torch.isfinite(dl).all()) and not dl.any()


@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('K,hw,HW', [CE_CASES[0], CE_CASES[3]])
def test_saturated_pixels(hip, K, hw, HW, route):
    """logits scaled until p is exactly 0 or 1 at some pixels (SAT_SCALE of the focal tests): e == 1 lands in the clamped bin NB - 1, every count is still exact, the loss is
    within 1 / NB of the sorted one, and loss, table and gradient are finite"""
    from segland_amd import ops
    preds, target = R.inputs(K, hw, HW)
    preds = preds * SAT_SCALE[K]
    e = R.errors(R.upsample(preds, target, torch.float32), target)[0]
    assert int((e == 1).sum()) >= 1 and int((e == 0).sum()) >= 1
    out, table, hist = lovasz_fwd(preds, target)
    h = hist.cpu().long()
    n_valid = int((target != 255).sum())
    assert h.sum((1, 2)).tolist() == [n_valid] * K and h[:, :, 0].sum(1).tolist() == [int((target == c).sum()) for c in range(K)]
    assert int(h[:, NB - 1].sum()) >= 1 and int(h[:, 0].sum()) >= 1
    exact = R.exact_sorted(preds, target)
    print('K %d saturated: loss %.8g (sorted %.8g), %d counts in the top bin' % (K, out[0].item(), exact, int(h[:, NB - 1].sum())))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(table).all()) and abs(out[0].item() - exact) <= 1.0 / NB
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    pg, tg = preds.to(DEV), target.to(DEV)
    ce = ops.upsample_ce_fwd(pg, tg, 255)
    dl = ops.upsample_lovasz_bwd(pg, tg, ce, None, table, torch.tensor([GS, 0.0, GS * MU], device=DEV), 255)
    assert bool(torch.isfinite(dl).all()) and float(dl.abs().max()) > 0


# --------------------------------------------------------------------------------------------- 6. OrthLoss
def _orth_inputs():
    K, HW = 8, (64, 64)
    preds, aux = fm.sym('lov/ol/preds', (2, K, 8, 8), 2.0), fm.sym('lov/ol/aux', (2, K, 16, 16), 1.5)
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='lov/ol/mask', block=8, ignore_rows=7)
    return K, preds, aux, target, fm.sym('lov/ol/sim', (4, 11), 1.0)


@pytest.mark.parametrize('kw', [dict(), dict(weight=True, label_smoothing=0.1, dice_weight=0.5, focal_gamma=2.0)])
def test_lovasz_weight_zero_is_the_criterion_without_it(hip, kw):
    from segland_amd.loss.criterion import OrthLoss
    K, preds, aux, target, sim = _orth_inputs()
    kw = dict(kw, weight=class_weights(K)) if kw.get('weight') else kw
    res = []
    for crit in (OrthLoss(255, **kw), OrthLoss(255, lovasz_weight=0.0, **kw)):
        crit = crit.to(DEV)
        pg, ag = preds.to(DEV).requires_grad_(True), aux.to(DEV).requires_grad_(True)
        d = crit(pg, target.to(DEV), is_ft=True, proto_sim=sim.to(DEV), aux_preds=ag)
        d['total_loss'].backward()
        res.append((d, pg.grad, ag.grad))
    (d0, p0, a0), (d1, p1, a1) = res
    assert list(d0) == list(d1) and 'lovasz_loss' not in d1
    assert all(torch.equal(d0[k], d1[k]) for k in d0) and torch.equal(p0, p1) and torch.equal(a0, a1)


@pytest.mark.parametrize('dice', [0.0, 0.5])
def test_orth_loss_with_lovasz_aux_and_rectangular_sim(hip, dice):
    """OrthLoss(weight, label_smoothing, [dice_weight], lovasz_weight 0.75): the dict gains 'lovasz_loss'; seg = ce [+ dice_weight dice] + 0.75 lovasz for both heads and
    total = seg + 10 orth + 0.4 aux, each term bit-equal to the ops called directly; the cross-entropy and Dice equal the criterion's without the term, bit for bit; the
    Lovasz terms lie within 1 / NB of the sorted loss; the gradients of both logit tensors equal the one-launch backward's"""
    from segland_amd import ops
    from segland_amd.loss.criterion import OrthLoss
    K, preds, aux, target, sim = _orth_inputs()
    w, eps, mu = class_weights(K), 0.1, 0.75
    crit = OrthLoss(255, weight=w, label_smoothing=eps, dice_weight=dice, lovasz_weight=mu).to(DEV)
    base = OrthLoss(255, weight=w, label_smoothing=eps, dice_weight=dice).to(DEV)
    assert len(crit.state_dict()) == 0
    pg, ag, tg = preds.to(DEV).requires_grad_(True), aux.to(DEV).requires_grad_(True), target.to(DEV)
    d = crit(pg, tg, is_ft=True, proto_sim=sim.to(DEV), aux_preds=ag)
    d0 = base(preds.to(DEV), tg, is_ft=True, proto_sim=sim.to(DEV), aux_preds=aux.to(DEV))
    assert list(d) == list(d0) + ['lovasz_loss']
    d['total_loss'].backward()
    lov, table = ops.upsample_lovasz_fwd(pg.detach(), tg, 255)
    lov_a, table_a = ops.upsample_lovasz_fwd(ag.detach(), tg, 255)
    assert torch.equal(d['lovasz_loss'], lov[0]) and torch.equal(d['orth_loss'], d0['orth_loss'])
    assert torch.equal(d['seg_loss'], torch.add(d0['seg_loss'], lov[0], alpha=mu)) and torch.equal(d['aux_loss'], torch.add(d0['aux_loss'], lov_a[0], alpha=mu))
    if dice:
        assert torch.equal(d['dice_loss'], d0['dice_loss'])
    assert torch.equal(d['total_loss'], d['seg_loss'] + d['orth_loss'] * 10.0 + 0.4 * d['aux_loss'])
    for x, l in ((preds, lov), (aux, lov_a)):
        exact = R.exact_sorted(x, target)
        print('lovasz %.8g (sorted %.8g)' % (l[0].item(), exact))
        assert abs(l[0].item() - exact) <= 1.0 / NB
    for x, got, tab, g_up in ((pg, pg.grad, table, 1.0), (ag, ag.grad, table_a, 0.4)):
        if dice:
            out, coef = ops.upsample_ce_dice_fwd(x.detach(), tg, 255, weight=crit.weight, label_smoothing=eps)
        else:
            out, coef = ops.upsample_ce_fwd(x.detach(), tg, 255, weight=crit.weight, label_smoothing=eps), None
        gs = torch.tensor([g_up, g_up * dice, g_up * mu], device=DEV)
        want = ops.upsample_lovasz_bwd(x.detach(), tg, out, coef, tab, gs, 255, 0.0, weight=crit.weight, label_smoothing=eps)
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize('lam', [0.0, 0.5])
def test_mining_runs_in_front_of_the_lovasz_term(hip, lam):
    """OrthLoss(ohem_thresh 0.7, small ohem_min_kept, lovasz_weight 0.5): loss and gradient equal, bit for bit, the ops run on the label map OrthLoss.mine returns, and the
    Lovasz term lies within 1 / NB of the sorted loss of the reference ON THE MINED MAP"""
    from segland_amd import ops
    from segland_amd.loss.criterion import OrthLoss
    r = R.case(8, (8, 8), (64, 64))
    w, mu = class_weights(8), 0.5
    crit = OrthLoss(255, weight=w, label_smoothing=0.1, dice_weight=lam, ohem_thresh=0.7, ohem_min_kept=300, lovasz_weight=mu).to(DEV)
    pg, tg = r['preds'].to(DEV).requires_grad_(True), r['target'].to(DEV)
    mined, frac = crit.mine(pg, tg)
    assert 0.0 < float(frac) < 1.0 and not torch.equal(mined, tg)
    seg, dice, frac2, lov = crit.head_terms(pg, tg)
    (seg * GS).backward()
    assert torch.equal(frac, frac2)
    kw = dict(weight=crit.weight, label_smoothing=0.1)
    l, table = ops.upsample_lovasz_fwd(pg.detach(), mined, 255)
    if lam:
        out, coef = ops.upsample_ce_dice_fwd(pg.detach(), mined, 255, **kw)
        assert torch.equal(seg.detach(), torch.add(torch.add(out[0], out[2], alpha=lam), l[0], alpha=mu)) and torch.equal(dice.detach(), out[2])
    else:
        out, coef = ops.upsample_ce_fwd(pg.detach(), mined, 255, **kw), None
        assert torch.equal(seg.detach(), torch.add(out[0], l[0], alpha=mu)) and dice is None
    assert torch.equal(lov.detach(), l[0])
    want = ops.upsample_lovasz_bwd(pg.detach(), mined, out, coef, table, torch.tensor([GS, GS * lam, GS * mu], device=DEV), 255, 0.0, **kw)
    assert torch.equal(pg.grad, want)
    exact = R.exact_sorted(r['preds'], mined.cpu())
    print('lovasz on the mined map %.8g (sorted %.8g; on the full map %.8g)' % (l[0].item(), exact, r['exact']))
    assert abs(l[0].item() - exact) <= 1.0 / NB and exact != r['exact']


# --------------------------------------------------------------------------------------------- 7. models
def _model(crit, **kw):
    from segland_amd.networks.pspnet_pop import GFSS_Model
    m = GFSS_Model(criterion=crit, backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=torch.float32, **kw)
    return fm.load_formula_weights(m).to(DEV)


@pytest.fixture
def lovasz_calls(monkeypatch):
    """names of the Lovasz ops in call order; the ops still run"""
    from segland_amd import ops
    seen = []
    for name in ('upsample_lovasz_fwd', 'upsample_lovasz_bwd'):
        def wrap(*a, _f=getattr(ops, name), _n=name, **kw):
            seen.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, wrap)
    return seen


def test_base_model_uses_the_lovasz_term(hip, lovasz_calls):
    """GFSS_Model(n_base=7) in train_mode() (backbone and decoder frozen), fp32, 2 x 64 x 64, lovasz_weight 0.5: the step reaches the Lovasz pair, lovasz_loss lies within
    1 / NB of the sorted loss on the logits of a criterion-less call of the same model; base_emb.grad is finite and non-zero"""
    from segland_amd.loss.criterion import OrthLoss
    K = 8
    m = _model(OrthLoss(255, weight=class_weights(K), label_smoothing=0.1, lovasz_weight=0.5), n_base=7)
    assert not any('criterion' in k for k in m.state_dict())
    m.train_mode()
    for part in (m.backbone, m.decoder):
        for p in part.parameters():
            p.requires_grad = False
    img = fm.formula_image(2, 64, 64, 'lov/img').to(DEV)
    mask = fm.formula_mask(2, 64, 64, K, 'lov/mask', block=8, ignore_rows=4)
    d = m(img, mask.to(DEV))
    d['total_loss'].backward()
    assert 'upsample_lovasz_fwd' in lovasz_calls and 'upsample_lovasz_bwd' in lovasz_calls and 'lovasz_loss' in d
    crit, m.criterion = m.criterion, None
    with torch.no_grad():
        logits = m(img).float().cpu()
    m.criterion = crit
    want = R.exact_sorted(logits, mask)
    print('base mode lovasz_loss %.8g (sorted loss on the model\'s logits %.8g)' % (float(d['lovasz_loss'].detach()), want))
    assert abs(float(d['lovasz_loss'].detach()) - want) <= 1.0 / NB
    g = m.base_emb.grad
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_ft_model_uses_the_lovasz_term(hip, lovasz_calls):
    """Fine-tune mode, 1 + 7 + 4 = 12 logit channels, one novel and one base tile (as test_focal_loss_gpu.test_ft_model_uses_the_focal_loss): the Lovasz pair is reached and
    lovasz_loss lies within 1 / NB of the sorted loss on the logits and the pseudo-labelled mask of a criterion-less call"""
    from segland_amd.loss.criterion import OrthLoss
    K = 12
    m = _model(None, n_base=7, is_ft=True, n_novel=4)
    m.init_cls_n()
    m.train_mode()
    img, img_b = fm.formula_image(1, 64, 64, 'lov/ftimg').to(DEV), fm.formula_image(1, 64, 64, 'lov/ftimg_b').to(DEV)
    mask = fm.formula_mask(1, 64, 64, 4, 'lov/ftmask', block=8, ignore_rows=4) + 8
    mask[mask > 11] = 255                                                        # novel ids 8..11
    mask_b = fm.formula_mask(1, 64, 64, 8, 'lov/ftmask_b', block=8, ignore_rows=0)     # background + 7 base classes
    mb = mask_b.clone().to(DEV)
    with torch.no_grad():
        logits = m(img, mask.to(DEV), img_b, mb).float().cpu()
    assert tuple(logits.shape) == (2, K, 8, 8)
    want = R.exact_sorted(logits, torch.cat([mask, mb.cpu()], 0))
    m.criterion = OrthLoss(255, weight=class_weights(K), dice_weight=0.5, lovasz_weight=0.5).to(DEV)
    mb2 = mask_b.clone().to(DEV)
    d = m(img, mask.to(DEV), img_b, mb2)
    assert torch.equal(mb2, mb)
    d['total_loss'].backward()
    assert 'upsample_lovasz_fwd' in lovasz_calls and 'upsample_lovasz_bwd' in lovasz_calls
    print('fine-tune mode lovasz_loss %.8g (sorted loss on the model\'s logits and pseudo-labels %.8g)' % (float(d['lovasz_loss'].detach()), want))
    assert abs(float(d['lovasz_loss'].detach()) - want) <= 1.0 / NB
    assert bool(torch.isfinite(m.novel_emb.grad).all()) and float(m.novel_emb.grad.abs().max()) > 0


def test_captured_step_with_lovasz_term_equals_eager(hip):
    """graph_step.GraphedTrainStep on PSPNet-POP fp32 (2 x 96 x 128, four batches, six steps) with class weights, Dice weight 0.5 and Lovasz weight 0.5 against the same
    steps issued kernel by kernel (losses, gradient norms, parameters: bit for bit, as test_focal_loss_gpu compares them); the last two steps are replays of one graph"""
    from segland_amd import graph_step
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    batches = [(fm.formula_image(2, 96, 128, 'lov/gs/img%d' % k).to(DEV), fm.formula_mask(2, 96, 128, 8, 'lov/gs/mask%d' % k, block=16, ignore_rows=4).to(DEV))
               for k in range(4)]
    ref = _model(OrthLoss(255, weight=class_weights(8), dice_weight=0.5, lovasz_weight=0.5), n_base=7).train()
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
            log.append((float(d['total_loss'].detach()), float(d['seg_loss'].detach()), float(d['dice_loss'].detach()), float(d['lovasz_loss'].detach()), float(gn)))
        if graphed:
            assert step.graph is not None and step.graph is graph_before and step.replays >= 2 and step.failures == 0, 'the last two steps were not replays of one graph'
        return log, {k: v.detach().float().cpu() for k, v in model.state_dict().items()}

    log_r, sd_r = run(ref, False)
    log_g, sd_g = run(got, True)
    print('losses / dice / lovasz / grad norms eager vs graph:', log_r, log_g)
    assert log_r == log_g
    assert all(np.isfinite(v) for row in log_r for v in row) and all(0.0 < row[3] <= 1.0 for row in log_r)
    for k in sd_r:
        assert torch.equal(sd_r[k], sd_g[k]), k
