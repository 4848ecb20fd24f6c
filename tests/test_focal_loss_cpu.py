"""Focal modulation of the fused upsample + loss criterion, CPU side: the four sl_upsample_focal_* entry points exist, are declared and validate before any launch;
OrthLoss keeps focal_gamma as a plain float (no buffer, no state_dict key) and refuses what is neither 0 nor a finite value >= 1; get_loss and both drivers' parsers carry
--focal-gamma and the log line names it only where it is on; focal_gamma == 0 never reaches a focal op; and the reference of the GPU tests (focal_reference.py) checks
itself: the header's closed-form gradient against float64 autograd, and mod == 1 against F.cross_entropy.  The kernels themselves: test_focal_loss_gpu.py."""
import argparse
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import focal_reference as R
from oracle import formula as fm


@pytest.fixture(scope='module')
def lib():
    from segland_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


ENTRIES = ('sl_upsample_focal_fwd', 'sl_upsample_focal_bwd', 'sl_upsample_focal_dice_fwd', 'sl_upsample_focal_dice_bwd')


def test_focal_entries_are_exported_and_declared(lib):
    from segland_amd import _lib
    decl = _lib.declared_functions()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in decl, name
        assert decl[name][1][3] is C.c_float and decl[name][1][4] is C.c_float, name          # label_smoothing, gamma
    assert [len(decl[n][1]) for n in ENTRIES] == [14, 16, 14, 17]
    # no existing signature gained an argument
    assert len(decl['sl_upsample_ce_fwd'][1]) == 11 and len(decl['sl_upsample_ce_bwd'][1]) == 13
    assert len(decl['sl_upsample_ce_weighted_fwd'][1]) == 13 and len(decl['sl_upsample_ce_weighted_bwd'][1]) == 15
    assert len(decl['sl_upsample_ce_dice_fwd'][1]) == 13 and len(decl['sl_upsample_ce_dice_bwd'][1]) == 16


def test_focal_entries_validate_before_any_launch(lib):
    """SL_EINVAL (-1) with a message and no launch (the pointers are not device memory: a launch would fault) for gamma below 1 or not finite, K = 34, a bad shape, a bad
    label smoothing and every null buffer; the message of a refused gamma holds the value"""
    d = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string().decode()
    calls = {
        'fwd': lambda gamma, K=8, eps=0.0, lg=d, t=d, out=d, H=64: lib.sl_upsample_focal_fwd(lg, t, None, eps, gamma, 2, K, 8, 8, H, 64, 255, out, None),
        'bwd': lambda gamma, K=8, eps=0.0, lg=d, t=d, out=d, H=64, lc=d, gs=d: lib.sl_upsample_focal_bwd(lg, t, None, eps, gamma, lc, gs, 2, K, 8, 8, H, 64, 255, out, None),
        'dice_fwd': lambda gamma, K=8, eps=0.0, lg=d, t=d, out=d, H=64: lib.sl_upsample_focal_dice_fwd(lg, t, None, eps, gamma, 2, K, 8, 8, H, 64, 255, out, None),
        'dice_bwd': lambda gamma, K=8, eps=0.0, lg=d, t=d, out=d, H=64, lc=d, gs=d, coef=d: lib.sl_upsample_focal_dice_bwd(lg, t, None, eps, gamma, lc, coef, gs, 2, K, 8, 8, H,
                                                                                                                       64, 255, out, None),
    }
    for name, call in calls.items():
        assert call(0.5) == -1 and 'gamma 0.5' in err() and '>= 1' in err(), name
        assert call(float('nan')) == -1 and 'gamma nan' in err(), name
        assert call(float('inf')) == -1 and 'gamma inf' in err(), name
        assert call(0.0) == -1 and 'gamma 0' in err(), name
        assert call(-2.0) == -1 and 'gamma -2' in err(), name
        assert call(2.0, K=34) == -1 and '34 logit channels' in err() and 'at most 33' in err(), name
        assert call(2.0, K=0) == -1 and 'at most 33' in err(), name
        assert call(2.0, eps=1.5) == -1 and 'label_smoothing' in err(), name
        assert call(2.0, H=0) == -1 and 'bad shape' in err(), name
        for buf in ('lg', 't', 'out'):
            assert call(2.0, **{buf: None}) == -1 and 'null' in err(), (name, buf)
    for name in ('bwd', 'dice_bwd'):
        for buf in ('lc', 'gs'):
            assert calls[name](2.0, **{buf: None}) == -1 and 'null' in err(), (name, buf)
    assert calls['dice_bwd'](2.0, coef=None) == -1 and 'null' in err()


def test_orth_loss_keeps_focal_gamma_as_a_plain_float():
    from segland_amd.loss.criterion import OrthLoss
    assert OrthLoss(255).focal_gamma == 0.0
    crit = OrthLoss(255, weight=[1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.75, 1.25], label_smoothing=0.1, dice_weight=0.5, focal_gamma=2)
    assert type(crit.focal_gamma) is float and crit.focal_gamma == 2.0
    assert [n for n, _ in crit.named_buffers()] == ['weight'] and not list(crit.parameters()) and len(crit.state_dict()) == 0
    assert OrthLoss(255, focal_gamma=1.0).focal_gamma == 1.0 and OrthLoss(255, focal_gamma=3.5).focal_gamma == 3.5
    assert len(OrthLoss(255, focal_gamma=2.0).state_dict()) == 0
    for bad in (0.5, -1.0, float('inf'), float('nan'), 0.999, -0.0001):
        with pytest.raises(ValueError, match='focal_gamma'):
            OrthLoss(255, focal_gamma=bad)
    from segland_amd.networks.pspnet_pop import GFSS_Model
    keys = lambda c: set(GFSS_Model(n_base=7, criterion=c, backbone='resnet50', pretrained_model=None, dilated=True, os=8).state_dict())
    assert keys(crit) == keys(OrthLoss(255)) == keys(None)


def test_get_loss_with_and_without_the_field():
    from segland_amd.loss import get_loss
    assert get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255)).focal_gamma == 0.0
    new = get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, class_weights=(1.0, 2.0, 0.5), dice_weight=0.5, focal_gamma=2.0))
    assert new.focal_gamma == 2.0 and new.dice_weight == 0.5 and new.weight.tolist() == [1.0, 2.0, 0.5]
    assert get_loss(argparse.Namespace(model='swin_pop', ignore_label=255, focal_gamma=1.5)).focal_gamma == 1.5
    with pytest.raises(ValueError):
        get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, focal_gamma=0.5))


@pytest.mark.parametrize('ft', [False, True])
def test_parsers_accept_the_focal_gamma(ft, capsys):
    from segland_amd.drivers import build_parser
    from segland_amd.loss import get_loss
    p = build_parser(ft)
    assert p.parse_args([]).focal_gamma == 0.0
    a = p.parse_args(['--focal-gamma', '2', '--model', 'pspnet_pop'])
    assert a.focal_gamma == 2.0
    a.ignore_label = 255
    assert get_loss(a).focal_gamma == 2.0
    assert p.parse_args(['--focal-gamma', '0']).focal_gamma == 0.0 and p.parse_args(['--focal-gamma', '1']).focal_gamma == 1.0
    for bad in ('0.5', '-1', 'nan', 'inf', 'x'):
        with pytest.raises(SystemExit):
            p.parse_args(['--focal-gamma', bad])
    capsys.readouterr()


def test_the_log_line_names_the_focal_gamma_only_where_it_is_on(caplog):
    import logging
    from segland_amd.drivers import build_parser, log_loss_options
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        log_loss_options(build_parser(False).parse_args(['--class-weights', '1,0.5', '--dice-weight', '0.5', '--focal-gamma', '2', '--ohem-thresh', '0.7']))
        log_loss_options(build_parser(True).parse_args(['--focal-gamma', '1.5']))
        log_loss_options(build_parser(False).parse_args(['--label-smoothing', '0.1']))
    assert [r.getMessage() for r in caplog.records] == [
        'segmentation loss: class weights 1,0.5, label smoothing 0, dice weight 0.5, focal gamma 2, hard-pixel mining: threshold 0.7, at least 100000 pixels per batch',
        'segmentation loss: class weights none, label smoothing 0, focal gamma 1.5',
        'segmentation loss: class weights none, label smoothing 0.1']


# --------------------------------------------------------------------------------------------- which ops a criterion reaches
@pytest.fixture
def calls(monkeypatch):
    """[op name, ...] in call order: the loss ops OrthLoss can reach are replaced by recorders that return zero tensors of the shapes the ops give (no GPU, no library)"""
    from segland_amd import ops
    seen = []

    def fwd(name, n):
        def f(logits, target, ignore_index, *a, **kw):
            seen.append(name)
            return torch.zeros(n) if n == 2 else (torch.zeros(3), torch.zeros(tuple(logits.shape[:2]) + (2,)))
        return f

    def bwd(name):
        def f(logits, *a, **kw):
            seen.append(name)
            return torch.zeros_like(logits)
        return f

    for name, n in (('upsample_ce_fwd', 2), ('upsample_ce_dice_fwd', 3), ('upsample_focal_fwd', 2), ('upsample_focal_dice_fwd', 3)):
        monkeypatch.setattr(ops, name, fwd(name, n))
        monkeypatch.setattr(ops, name.replace('_fwd', '_bwd'), bwd(name.replace('_fwd', '_bwd')))
    return seen


def _one_step(crit):
    preds = torch.zeros(2, 8, 4, 4, requires_grad=True)
    d = crit(preds, torch.zeros(2, 16, 16, dtype=torch.int64), proto_sim=torch.ones(3, 3), aux_preds=torch.zeros(2, 8, 4, 4, requires_grad=True))
    d['total_loss'].backward()
    return d


def test_focal_gamma_zero_never_reaches_a_focal_op(calls, monkeypatch):
    """focal_gamma == 0 is the code path without it: with the four focal ops patched to raise, the plain and the hybrid criterion still run, on the ops they ran on"""
    from segland_amd import ops
    from segland_amd.loss.criterion import OrthLoss

    def boom(*a, **kw):
        raise AssertionError('a focal op was reached with focal_gamma == 0')
    for name in ('upsample_focal_fwd', 'upsample_focal_bwd', 'upsample_focal_dice_fwd', 'upsample_focal_dice_bwd'):
        monkeypatch.setattr(ops, name, boom)
    assert list(_one_step(OrthLoss(255, focal_gamma=0.0))) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss']
    assert sorted(calls) == ['upsample_ce_bwd'] * 2 + ['upsample_ce_fwd'] * 2
    del calls[:]
    assert list(_one_step(OrthLoss(255, dice_weight=0.5, focal_gamma=0))) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss', 'dice_loss']
    assert sorted(calls) == ['upsample_ce_dice_bwd'] * 2 + ['upsample_ce_dice_fwd'] * 2


def test_focal_gamma_routes_both_heads_to_the_focal_ops(calls):
    """on: main and auxiliary head run the focal pair (the focal hybrid pair with dice_weight > 0) and nothing else; the dict gains no key"""
    from segland_amd.loss.criterion import OrthLoss
    assert list(_one_step(OrthLoss(255, focal_gamma=2.0))) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss']
    assert sorted(calls) == ['upsample_focal_bwd'] * 2 + ['upsample_focal_fwd'] * 2
    del calls[:]
    assert list(_one_step(OrthLoss(255, dice_weight=0.5, focal_gamma=1.0))) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss', 'dice_loss']
    assert sorted(calls) == ['upsample_focal_dice_bwd'] * 2 + ['upsample_focal_dice_fwd'] * 2


def test_focal_ops_refuse_cpu_tensors(lib):
    from segland_amd import ops
    lg, t = torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 16, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='not on the GPU'):
        ops.upsample_focal_fwd(lg, t, 255, 2.0)
    with pytest.raises(RuntimeError, match='not on the GPU'):
        ops.upsample_focal_dice_fwd(lg, t, 255, 2.0)
    with pytest.raises(RuntimeError, match='not on the GPU'):
        ops.upsample_focal_bwd(lg, t, torch.zeros(2), torch.ones(1), 255, 2.0)
    with pytest.raises(RuntimeError, match='not on the GPU'):
        ops.upsample_focal_dice_bwd(lg, t, torch.zeros(3), torch.zeros(2, 8, 2), torch.ones(2), 255, 2.0)


# --------------------------------------------------------------------------------------------- the reference checks itself
def _pixels(K, n=200, scale=4.0):
    v = fm.sym('focal/cpu/v%d' % K, (n, K), scale).double()
    t = (fm.uniform01('focal/cpu/t%d' % K, n) * K).floor().to(torch.int64).clamp(max=K - 1)
    w = (1.25 + fm.sym('focal/cpu/w%d' % K, (K,), 0.75)).double()
    w[K // 2] = 0.0
    return v, t, w


@pytest.mark.parametrize('gamma', [1.0, 2.0, 3.5])
@pytest.mark.parametrize('weighted,eps', [(False, 0.0), (True, 0.0), (True, 0.1)])
@pytest.mark.parametrize('K', [8, 33])
def test_closed_form_gradient_equals_float64_autograd(K, weighted, eps, gamma):
    """d / d v_k = mod * ceform_k + beta * (p_k - [k == t]) of the header against autograd of the definition, float64, 1e-12 of the largest entry"""
    v, t, w = _pixels(K)
    w = w if weighted else None
    vr = v.clone().requires_grad_(True)
    mod, num0, _ = R.pixel_terms(vr, t, gamma, w, eps)
    (mod * num0).sum().backward()
    got = R.closed_form_grad(v, t, gamma, w, eps)
    err = float((got - vr.grad).abs().max() / vr.grad.abs().max())
    print('K %d weighted %s eps %g gamma %g: closed form vs autograd %.3g relative' % (K, weighted, eps, gamma, err))
    assert err <= 1e-12


@pytest.mark.parametrize('weighted,eps', [(False, 0.0), (True, 0.0), (True, 0.1)])
def test_reference_with_mod_one_is_cross_entropy(weighted, eps):
    """mod == 1 (gamma 0 of the reference): loss and weight sum of F.cross_entropy(weight, ignore_index, label_smoothing) on the same upsampled logits, float64"""
    K, HW = 8, (40, 33)
    logits = fm.sym('focal/cpu/p', (2, K, 9, 7), 3.0).double()
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='focal/cpu/m', block=8, ignore_rows=5)
    w = _pixels(K)[2] if weighted else None
    up = R.upsample(logits, HW)
    loss, wsum = R.focal_loss(up, target, 0, w, eps)
    want = F.cross_entropy(up, target, weight=w, ignore_index=255, label_smoothing=eps)
    valid = target[target != 255]
    assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want))
    assert abs(float(wsum) - (float(w[valid].sum()) if weighted else valid.numel())) <= 1e-12 * float(wsum)


def test_kernel_u_replay_saturates_where_the_other_classes_underflow():
    """u of the float32 replay: exactly 0 where every other exponential underflows, 1 - p_t elsewhere (against float64)"""
    up = torch.tensor([[200.0, 0.0, -3.0], [0.5, 0.25, 0.0], [-120.0, 0.0, -110.0]]).T.reshape(1, 3, 1, 3).contiguous()
    target = torch.tensor([[[0, 1, 1]]])
    u = R.kernel_u(up, target)
    assert u[0] == 0.0 and 0.0 < u[1] < 1.0
    p = up.double().softmax(1)[0, :, 0, :]
    assert abs(u[1] - (1.0 - float(p[1, 1]))) < 1e-6 and abs(u[2] - (1.0 - float(p[1, 2]))) < 1e-6
