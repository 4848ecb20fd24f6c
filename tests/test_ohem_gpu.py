"""Online hard-pixel mining (OHEM) in the fused upsample + loss path: the three passes of csrc/loss.hip (sl_upsample_ohem_prob, sl_ohem_threshold, sl_ohem_mine), ops.ohem_mine,
OrthLoss(ohem_thresh, ohem_min_kept), the PSPNet-POP model in fine-tune mode and a captured training step, against the definition in torch on the CPU
(tests/ohem_reference.py).

Conditions on the INPUTS, asserted on the CPU in every case that compares kept sets: no valid probability lies within 1e-5 of theta other than q and its exact ties
(ohem_reference.GAP), a binding q is no tie of two different pixels, and 8 x max |prob_gpu - p_cpu| stays below that gap (printed).  Under them the kept set of the kernels
is the reference's, bit for bit, and everything after it compares at the bounds of tests/test_weighted_ce_gpu.py and tests/test_dice_loss_gpu.py.

Without the feature every test but the default-off one fails (missing ops / unexpected keyword)."""
import copy
import functools

import numpy as np
import pytest
import torch

import ohem_reference as R
from oracle import formula as fm
from test_dice_loss_gpu import class_weights

pytestmark = pytest.mark.gpu
DEV = 'cuda'
THRESH = 0.7
# regime -> how the inputs are built: 'thresh' random logits, theta = thresh; 'min_kept' mostly-right logits and a min_kept half way between the pixels at or below the
# threshold and n, theta = q > thresh; 'one' random logits, min_kept = 1
REGIMES = ['thresh', 'min_kept', 'one']


@functools.lru_cache(maxsize=None)
def kernel_case(K, hw, HW, regime):
    """the formula inputs with salt 0 meet the conditions on the inputs at every shape and regime (asserted where they are used); another salt gives other inputs"""
    target = R.labels('k', K, HW)
    if regime == 'min_kept':
        logits = R.mostly_right_logits('k', K, hw, target)
        p, valid = R.true_class_prob(logits, target)
        n, n_le = int(valid.sum()), int((p <= THRESH).sum())
        min_kept = n_le + (n - n_le) // 2
    else:
        logits = R.random_logits('k', K, hw)
        min_kept = 1 if regime == 'one' else max(int((target != 255).sum()) // 64, 2)
    rec = R.mine(logits, target, THRESH, min_kept)
    return dict(logits=logits, target=target, min_kept=min_kept, rec=rec)


def assert_input_conditions(rec, binds, what):
    print('%s: n %d, k %d, q %.8g, theta %.8g, kept %d, gap around theta %.3g, ties at q %d' % (what, rec['n'], rec['k'], rec['q'], rec['theta'], rec['n_kept'], rec['gap'], rec['ties']))
    assert rec['binds'] == binds, 'the case is in the other regime'
    assert rec['gap'] >= R.GAP, 'a probability within %g of theta: choose another salt' % R.GAP
    assert not binds or rec['ties'] == 1, 'q is a tie of different pixels: choose another salt'


def mine_twice(lg, tg, thresh, min_kept):
    """ops.ohem_mine and the probability pass, twice: two runs must give the same bits, and the target is not written"""
    from segland_amd import ops
    before = tg.clone()
    a = ops.ohem_mine(lg, tg, 255, thresh, min_kept)
    b = ops.ohem_mine(lg, tg, 255, thresh, min_kept)
    pa, pb = ops.ohem_prob(lg, tg, 255), ops.ohem_prob(lg, tg, 255)
    for x, y in zip(a + (pa,), b + (pb,)):
        assert torch.equal(x, y), 'run to run'
    assert torch.equal(tg, before), 'the target was written'
    mined, theta, counts = a
    assert mined.dtype == torch.int64 and mined.shape == tg.shape and mined.data_ptr() != tg.data_ptr()
    return mined.cpu(), float(theta.cpu()[0]), [int(c) for c in counts.cpu()], pa.cpu()


def check_kernels(rec, mined, theta, counts, prob, what):
    err = float((prob - rec['p'])[rec['valid']].abs().max()) if rec['n'] else 0.0
    print('%s: max |prob - p| %.3g (8 x that must stay below the gap %.3g), theta %.9g (torch %.9g)' % (what, err, rec['gap'], theta, rec['theta']))
    assert bool((prob[~rec['valid']] == 2.0).all()), 'sentinel'
    assert 8.0 * err < rec['gap']
    assert counts == [rec['n'], rec['k'], rec['n_kept']]
    assert torch.equal(mined, rec['mined'])
    np.testing.assert_allclose(theta, rec['theta'], rtol=2e-6)


# --------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('K,hw,HW', R.SHAPES)
def test_mining_kernels(hip, K, hw, HW, regime):
    """n, k, n_kept exact, the mined map torch.equal, theta rtol 2e-6, the sentinel on the pixels that are not valid, two runs the same bits; both regimes and min_kept = 1"""
    c = kernel_case(K, hw, HW, regime)
    what = 'K %d %s -> %s, %s' % (K, hw, HW, regime)
    assert_input_conditions(c['rec'], regime == 'min_kept', what)
    out = mine_twice(c['logits'].to(DEV), c['target'].to(DEV), THRESH, c['min_kept'])
    check_kernels(c['rec'], *out, what)


# --------------------------------------------------------------------------------------------- 2. ties
def test_all_ties_at_q_are_kept(hip):
    """Identity scale, four kinds of pixel (label j, logit level L_j at channel j and 0 elsewhere): hundreds of pixels share each probability bit for bit.  min_kept in
    the middle of the second group: the whole group is kept, n_kept is the CPU count."""
    K, S = 8, 24
    kind = (fm.uniform01('ohem/ties/kind', 2 * S * S) * 4).floor().long().reshape(2, S, S)
    level = torch.tensor([-2.0, 0.5, 2.5, 5.0])
    logits = (torch.nn.functional.one_hot(kind, K).float() * level[kind][..., None]).permute(0, 3, 1, 2).contiguous()
    target = kind.clone()
    target[0, :5] = 255
    sizes = [int((target == j).sum()) for j in range(4)]
    assert min(sizes) >= 200
    min_kept = sizes[0] + sizes[1] // 2
    rec = R.mine(logits, target, 0.1, min_kept)
    assert rec['binds'] and rec['ties'] == sizes[1] and rec['n_kept'] == sizes[0] + sizes[1] and rec['gap'] >= R.GAP
    assert torch.equal(rec['kept'], (target == 0) | (target == 1))
    mined, theta, counts, prob = mine_twice(logits.to(DEV), target.to(DEV), 0.1, min_kept)
    assert all(len(prob[target == j].unique()) == 1 for j in range(4)), 'the pixels of one kind do not share their probability bit for bit'
    check_kernels(rec, mined, theta, counts, prob, 'ties: groups of %s, min_kept %d' % (sizes, min_kept))
    assert counts[2] == sizes[0] + sizes[1] and torch.equal(mined != 255, (target == 0) | (target == 1))


# --------------------------------------------------------------------------------------------- 3. degenerate ends
ENDS = ['min_kept>=n', 'thresh=1', 'labels 250', 'sample 1 ignored', 'all ignored']


@pytest.mark.parametrize('end', ENDS)
@pytest.mark.parametrize('K,hw,HW', R.SHAPES)
def test_degenerate_ends_are_the_plain_path(hip, K, hw, HW, end):
    """Where nothing is dropped, mined equals the target on the valid pixels and the loss and dlogits of the plain kernels on it are torch.equal to those on the target"""
    from segland_amd import ops
    c = kernel_case(K, hw, HW, 'thresh')
    lg, target = c['logits'].to(DEV), c['target'].clone()
    thresh, min_kept = THRESH, 1 << 40
    if end == 'thresh=1':
        thresh, min_kept = 1.0, 1
    elif end == 'labels 250':
        target[1, 1:HW[0] // 2, 2:HW[1] - 1] = 250
        target[1, 0, 0] = -3
    elif end == 'sample 1 ignored':
        target[1] = 255
    elif end == 'all ignored':
        target[:] = 255
    valid = (target >= 0) & (target < K)
    n = int(valid.sum())
    tg = target.to(DEV)
    mined, theta, counts, prob = mine_twice(lg, tg, thresh, min_kept)
    assert counts == [n, min(min_kept, n), n]
    assert bool((prob[~valid] == 2.0).all()) and bool((prob[valid] <= 1.0).all())
    if end == 'all ignored':
        assert n == 0 and torch.equal(mined, target) and theta == np.float32(thresh)
        return
    assert n > 0 and torch.equal(mined[valid], target[valid]) and bool((mined[~valid] == 255).all())
    one = torch.ones(1, device=DEV)
    res = []
    for t in (tg, mined.to(DEV)):
        out = ops.upsample_ce_fwd(lg, t, 255)
        res.append((out, ops.upsample_ce_bwd(lg, t, out, one, 255)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and bool(torch.isfinite(res[0][1]).all())


# --------------------------------------------------------------------------------------------- 4. OrthLoss
MODES = {'plain': dict(), 'weights+smoothing': dict(weighted=True, eps=0.1), 'dice': dict(weighted=True, eps=0.1, lam=0.5)}


@functools.lru_cache(maxsize=None)
def criterion_case(mode):
    """main head: mostly-right logits on which min_kept binds; auxiliary head: random logits on which the threshold decides (same min_kept); a [4, 11] proto_sim.
    The CPU composition in float32 (the reference) and in float64 on the float32 kept sets (the reference's own error)."""
    K, HW = 8, (64, 64)
    kw = MODES[mode]
    w = class_weights(K) if kw.get('weighted') else None
    eps, lam = kw.get('eps', 0.0), kw.get('lam', 0.0)
    target = R.labels('c', K, HW)
    preds, aux = R.mostly_right_logits('c', K, (8, 8), target), R.random_logits('c/aux', K, (16, 16))
    p, valid = R.true_class_prob(preds, target)
    n, n_le = int(valid.sum()), int((p <= THRESH).sum())
    min_kept = n_le + (n - n_le) // 2
    sim = fm.sym('ohem/c/sim', (4, 11), 1.0)

    def compose(dtype, fixed=None):
        pr, ar = preds.to(dtype).clone().requires_grad_(True), aux.to(dtype).clone().requires_grad_(True)
        if fixed is None:
            seg, dice, rec_m = R.head_loss(pr, target, THRESH, min_kept, w, eps, lam)
            auxl, _, rec_a = R.head_loss(ar, target, THRESH, min_kept, w, eps, lam)
        else:                                           # the kept sets are constants: the float64 composition runs on the float32 ones
            seg, dice, _ = R.head_loss(pr, fixed[0]['mined'], None, 0, w, eps, lam)
            auxl, _, _ = R.head_loss(ar, fixed[1]['mined'], None, 0, w, eps, lam)
            rec_m, rec_a = fixed
        s = sim.to(dtype)
        orth = s[torch.triu(torch.ones_like(s), diagonal=1) == 1].abs().mean()
        ref = {'seg_loss': seg, 'aux_loss': auxl, 'orth_loss': orth, 'total_loss': seg + orth * 10.0 + 0.4 * auxl}
        if dice is not None:
            ref['dice_loss'] = dice
        ref['total_loss'].backward()
        return {k: float(v.detach()) for k, v in ref.items()}, pr.grad.numpy(), ar.grad.numpy(), rec_m, rec_a

    ref, gp, ga, rec_m, rec_a = compose(torch.float32)
    _, gp64, ga64, _, _ = compose(torch.float64, (rec_m, rec_a))
    ref['ohem_frac'] = float(torch.tensor(rec_m['n_kept'] / rec_m['n'], dtype=torch.float64).float())
    floors = []
    for rec in (rec_m, rec_a):                          # the floors of the weighted test on the KEPT pixels: they are the denominator now
        kept = target[rec['kept']]
        floors.append(2e-8 * (float(w.max()) * kept.numel() / float(w.double()[kept].sum()) if w is not None else 1.0))
    return dict(preds=preds, aux=aux, target=target, sim=sim, w=w, eps=eps, lam=lam, min_kept=min_kept, ref=ref, gp=gp, ga=ga, rec_m=rec_m, rec_a=rec_a, floors=floors,
                oracle_err=(float(np.abs(gp - gp64).max()), float(np.abs(ga - ga64).max())))


@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('mode', list(MODES))
def test_orth_loss_with_mining(hip, mode, route):
    """Every dict entry rtol 2e-5 against the CPU composition, the gradients of both logit tensors rtol 1e-3 with the absolute floors of the weighted test (plain,
    weights + smoothing) and of the hybrid test (dice: the larger of that floor and 8 x the reference's own float32 error), ohem_frac = n_kept / n of the main head"""
    from segland_amd import ops
    from segland_amd.loss.criterion import OrthLoss
    c = criterion_case(mode)
    assert_input_conditions(c['rec_m'], True, '%s, main head' % mode)
    assert_input_conditions(c['rec_a'], False, '%s, auxiliary head' % mode)
    for lg, rec in ((c['preds'], c['rec_m']), (c['aux'], c['rec_a'])):
        err = float((ops.ohem_prob(lg.to(DEV), c['target'].to(DEV), 255).cpu() - rec['p'])[rec['valid']].abs().max())
        assert 8.0 * err < rec['gap'], (err, rec['gap'])
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    crit = OrthLoss(255, weight=c['w'], label_smoothing=c['eps'], dice_weight=c['lam'], ohem_thresh=THRESH, ohem_min_kept=c['min_kept']).to(DEV)
    assert len(crit.state_dict()) == 0
    pg, ag, tg = c['preds'].to(DEV).requires_grad_(True), c['aux'].to(DEV).requires_grad_(True), c['target'].to(DEV)
    before = tg.clone()
    d = crit(pg, tg, is_ft=True, proto_sim=c['sim'].to(DEV), aux_preds=ag)
    d['total_loss'].backward()
    assert torch.equal(tg, before) and sorted(d) == sorted(c['ref'])
    for k, v in c['ref'].items():
        print('%s: %.8g (torch %.8g)' % (k, float(d[k].detach()), v))
        np.testing.assert_allclose(float(d[k].detach()), v, rtol=2e-5, err_msg=k)
    assert float(d['ohem_frac']) == c['ref']['ohem_frac'] and 0.0 < c['ref']['ohem_frac'] < 1.0
    for name, got, want, floor, oerr in (('preds', pg.grad, c['gp'], c['floors'][0], c['oracle_err'][0]), ('aux_preds', ag.grad, c['ga'], c['floors'][1], c['oracle_err'][1])):
        atol = max(floor, 8.0 * oerr) if mode == 'dice' else floor
        print('   d total / d %s: max abs error %.3g, floor %.3g (max |grad| %.3g, torch fp32 is %.2g absolute from float64)'
              % (name, float(np.abs(got.cpu().numpy() - want).max()), atol, float(np.abs(want).max()), oerr))
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-3, atol=atol)


def test_reduce_loss_dict_carries_ohem_frac(hip):
    """engine.reduce_loss_dict and the drivers' log line iterate the dict: ohem_frac comes through as a float under its key"""
    from segland_amd.engine import Engine
    from segland_amd.loss.criterion import OrthLoss
    c = criterion_case('plain')
    d = OrthLoss(255, ohem_thresh=THRESH, ohem_min_kept=c['min_kept']).to(DEV)(c['preds'].to(DEV), c['target'].to(DEV), proto_sim=c['sim'].to(DEV))
    eng = Engine.__new__(Engine)
    eng.distributed, eng.world_size = False, 1
    vals = eng.reduce_loss_dict(d)
    assert list(vals) == list(d) == ['total_loss', 'seg_loss', 'orth_loss', 'ohem_frac']
    assert ' ohem_frac=%.4f' % c['ref']['ohem_frac'] in ''.join(' %s=%.4f' % kv for kv in vals.items())


# --------------------------------------------------------------------------------------------- 5. the caller's target; fine-tune mode
def _model(crit, **kw):
    from segland_amd.networks.pspnet_pop import GFSS_Model
    m = GFSS_Model(criterion=crit, backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=torch.float32, **kw)
    return fm.load_formula_weights(m).to(DEV)


def test_ft_model_mines_on_a_copy_of_the_pseudo_labels(hip):
    """Fine-tune mode, 1 + 7 + 4 logit channels, one novel and one base tile (as test_weighted_ce_gpu.test_ft_model_uses_the_weighted_loss): mask_b after the call with
    mining equals mask_b after the same call without it (forward_novel hands the pseudo-labelled mask back in place; the mined map is a buffer of its own), and seg_loss
    equals the CPU reference on the model's own logits and that mask (rtol 2e-5).  The threshold is the middle of the widest gap between neighbouring probabilities (from
    the CPU reference on those logits; the formula-weight model puts them near 0 and near 1), min_kept = 1: a proper subset is kept."""
    from segland_amd.loss.criterion import OrthLoss
    K = 12
    m = _model(None, n_base=7, is_ft=True, n_novel=4)
    m.init_cls_n()
    m.train_mode()
    img, img_b = fm.formula_image(1, 64, 64, 'ohem/ftimg').to(DEV), fm.formula_image(1, 64, 64, 'ohem/ftimg_b').to(DEV)
    mask = fm.formula_mask(1, 64, 64, 4, 'ohem/ftmask', block=8, ignore_rows=4) + 8
    mask[mask > 11] = 255
    mask_b = fm.formula_mask(1, 64, 64, 8, 'ohem/ftmask_b', block=8, ignore_rows=0)
    mb = mask_b.clone().to(DEV)
    with torch.no_grad():
        logits = m(img, mask.to(DEV), img_b, mb).float().cpu()
    assert tuple(logits.shape) == (2, K, 8, 8)
    mask_all = torch.cat([mask, mb.cpu()], 0)
    assert int((mb.cpu() != mask_b).sum()) > 0, 'no pseudo-label was written: the case checks less than it says'
    p, valid = R.true_class_prob(logits, mask_all)
    pv = p[valid].sort().values
    n = pv.numel()
    i = int((pv[1:] - pv[:-1]).argmax())
    thresh = float((pv[i].double() + pv[i + 1].double()) / 2)
    seg, _, rec = R.head_loss(logits, mask_all, thresh, 1)
    assert_input_conditions(rec, False, 'fine-tune mode, thresh %.8g' % thresh)
    assert rec['n_kept'] == i + 1 and 0 < rec['n_kept'] < n
    m.criterion = OrthLoss(255, ohem_thresh=thresh, ohem_min_kept=1).to(DEV)
    mb2 = mask_b.clone().to(DEV)
    d = m(img, mask.to(DEV), img_b, mb2)
    assert torch.equal(mb2, mb), 'mask_b differs from the call without mining'
    print('fine-tune mode seg_loss %.8g (CPU reference on the model\'s logits and pseudo-labels %.8g), ohem_frac %.6f (%d / %d)'
          % (float(d['seg_loss'].detach()), float(seg), float(d['ohem_frac']), rec['n_kept'], n))
    np.testing.assert_allclose(float(d['seg_loss'].detach()), float(seg), rtol=2e-5)
    assert float(d['ohem_frac']) == float(torch.tensor(rec['n_kept'] / n, dtype=torch.float64).float())
    d['total_loss'].backward()
    assert bool(torch.isfinite(m.novel_emb.grad).all()) and float(m.novel_emb.grad.abs().max()) > 0


# --------------------------------------------------------------------------------------------- 6. default off
def test_off_is_the_path_without_it(hip, monkeypatch):
    """OrthLoss(255) and OrthLoss(255, ohem_thresh=None) (and 0): the same keys, torch.equal values and gradients, and the mining op is never called"""
    from segland_amd import ops
    from segland_amd.loss.criterion import OrthLoss

    def boom(*a, **k):
        raise AssertionError('ops.ohem_mine called with mining off')
    monkeypatch.setattr(ops, 'ohem_mine', boom)
    c = criterion_case('plain')
    res = []
    for crit in (OrthLoss(255), OrthLoss(255, ohem_thresh=None), OrthLoss(255, ohem_thresh=0, ohem_min_kept=5)):
        pg, ag = c['preds'].to(DEV).requires_grad_(True), c['aux'].to(DEV).requires_grad_(True)
        d = crit.to(DEV)(pg, c['target'].to(DEV), is_ft=True, proto_sim=c['sim'].to(DEV), aux_preds=ag)
        d['total_loss'].backward()
        res.append((d, pg.grad, ag.grad))
    for d, gp, ga in res[1:]:
        assert list(d) == list(res[0][0]) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss']
        for k in d:
            assert torch.equal(d[k], res[0][0][k]), k
        assert torch.equal(gp, res[0][1]) and torch.equal(ga, res[0][2])


# --------------------------------------------------------------------------------------------- 7. captured step
def test_captured_step_with_mining_equals_eager(hip):
    """graph_step.GraphedTrainStep on PSPNet-POP fp32 (2 x 96 x 128, four different batches, six steps) with ohem_thresh 0.7 against the same steps issued kernel by
    kernel, compared as test_dice_loss_gpu.test_captured_step_with_hybrid_loss_equals_eager compares them (bit for bit); the last two steps are replays of one graph.
    The classifier's last layer is scaled by 8, so that the formula-weight model is confident about part of the pixels (unscaled, no probability passes 0.7); in the CPU
    oracle of that model at its initial weights 23805 / 23399 / 23722 / 23332 of the 24064 valid pixels of the four batches lie at or below 0.7, and min_kept = 23560 lies
    between them.  The weights move with every step, so which steps bind is read from ohem_frac itself: it is min_kept / n where min_kept binds and larger where the
    threshold decides, both occur, and it changes from one replayed step to the next, which shows that a replay mines again."""
    from segland_amd import graph_step
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    N, MIN_KEPT = 24064, 23560
    batches = [(fm.formula_image(2, 96, 128, 'ohem/gs/img%d' % k).to(DEV), fm.formula_mask(2, 96, 128, 8, 'ohem/gs/mask%d' % k, block=16, ignore_rows=4).to(DEV))
               for k in range(4)]
    assert all(int((m != 255).sum()) == N for _, m in batches)
    ref = _model(OrthLoss(255, ohem_thresh=THRESH, ohem_min_kept=MIN_KEPT), n_base=7).train()
    with torch.no_grad():
        ref.classifier[4].weight.mul_(8.0)
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
            log.append((float(d['total_loss'].detach()), float(d['seg_loss'].detach()), float(d['ohem_frac'].detach()), float(gn)))
        if graphed:
            assert step.graph is not None and step.graph is graph_before and step.replays >= 2 and step.failures == 0, 'the last two steps were not replays of one graph'
        return log, {k: v.detach().float().cpu() for k, v in model.state_dict().items()}

    log_r, sd_r = run(ref, False)
    log_g, sd_g = run(got, True)
    print('losses / ohem_frac / grad norms eager vs graph:', log_r, log_g)
    assert log_r == log_g
    assert all(np.isfinite(v) for row in log_r for v in row)
    fracs = [row[2] for row in log_r]
    bound = float(torch.tensor(MIN_KEPT / N, dtype=torch.float64).float())
    assert all(bound <= f <= 1.0 for f in fracs) and any(f == bound for f in fracs) and any(f > bound for f in fracs), fracs
    assert len(set(fracs[2:])) > 1, 'ohem_frac of the replayed steps does not change with the batch'
    for k in sd_r:
        assert torch.equal(sd_r[k], sd_g[k]), k


@pytest.mark.parametrize('ft', [False, True])
def test_drivers_train_with_mining(hip, tmp_path, caplog, ft):
    """train_base / ft_pop on the synthetic set (the flags of tests/test_drivers_gpu.py) with --ohem-thresh 0.7 --ohem-min-kept 1000: the start-up line names the mining
    controls, the step log carries ohem_frac in (0, 1], a checkpoint with finite weights is written"""
    import glob
    import logging
    import os
    import re
    from segland_amd import ft_pop, train_base
    snap = str(tmp_path / 'snap')
    common = ['--model', 'pspnet_pop', '--backbone', 'resnet50', '--dataset', 'synthetic', '--input-size', '128,128', '--base-size', '128,128', '--num-epoch', '1',
              '--snapshot-dir', snap, '--num-workers', '0', '--restore-from', '/nonexistent', '--allow-random-init', '--ohem-thresh', '0.7', '--ohem-min-kept', '1000']
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        if ft:
            ft_pop.main(common + ['--batch-size', '1', '--learning-rate', '1e-3', '--print-frequency', '5', '--random-seed', '123', '--freeze-backbone', '--fix-bn'])
        else:
            train_base.main(common + ['--batch-size', '4', '--learning-rate', '1e-4', '--print-frequency', '4', '--fp16'])
    text = '\n'.join(r.getMessage() for r in caplog.records)
    assert 'hard-pixel mining: threshold 0.7, at least 1000 pixels per batch' in text
    fracs = [float(x) for x in re.findall(r' ohem_frac=([0-9.]+)', text)]
    assert len(fracs) >= 1 and all(0.0 < f <= 1.0 for f in fracs), text[-2000:]
    ck = glob.glob(os.path.join(snap, 'epoch_0_123.pth' if ft else 'epoch_1.pth'))
    assert ck, 'no checkpoint written'
    assert all(torch.isfinite(v.float()).all() for v in torch.load(ck[0], map_location='cpu').values())


# --------------------------------------------------------------------------------------------- 8. bad arguments
def test_bad_arguments_are_refused_before_any_launch(hip):
    from segland_amd import ops
    c = kernel_case(8, (8, 8), (64, 64), 'thresh')
    lg, tg = c['logits'].to(DEV), c['target'].to(DEV)
    for thresh in (0.0, 1.5):
        with pytest.raises(RuntimeError, match=r'thresh .* outside \(0, 1\]'):
            ops.ohem_mine(lg, tg, 255, thresh, 10)
    with pytest.raises(RuntimeError, match='min_kept 0 is not >= 1'):
        ops.ohem_mine(lg, tg, 255, 0.7, 0)
    with pytest.raises(RuntimeError, match='34 logit channels; this build holds at most 33'):
        ops.ohem_mine(torch.zeros(1, 34, 4, 4, device=DEV), torch.zeros(1, 8, 8, dtype=torch.int64, device=DEV), 255, 0.7, 1)
    prob = ops.ohem_prob(lg, tg, 255)
    need = hip.sl_ohem_workspace(2, 64, 64)
    assert need > 0 and hip.sl_ohem_workspace(0, 64, 64) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    theta, counts = torch.full((1,), -1.0, device=DEV), torch.full((3,), -1, dtype=torch.int64, device=DEV)
    args = lambda nbytes: (prob.data_ptr(), prob.numel(), 0.7, 10, ws.data_ptr(), nbytes, theta.data_ptr(), counts.data_ptr(), None)
    assert hip.sl_ohem_threshold(*args(need - 1)) == -1 and b'workspace' in hip.sl_last_error_string()
    assert hip.sl_ohem_threshold(prob.data_ptr(), prob.numel(), 0.7, 10, None, need, theta.data_ptr(), counts.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert float(theta[0]) == -1.0 and counts.tolist() == [-1, -1, -1], 'a refused call wrote its outputs'
