"""Lovasz-softmax term of the fused upsample + loss criterion, CPU side: the reference of the GPU tests (lovasz_reference.py) checks itself -- the binned loss against
the textbook sorted one within the derived 1 / (2 NB), the closed-form gradient against float64 autograd -- and states the conditions on the test inputs that keep the GPU
tests' slack honest; the five sl_*lovasz* entry points exist, are declared and validate before any launch; OrthLoss keeps lovasz_weight as a plain float and refuses what
is not a finite value >= 0; get_loss and both drivers' parsers carry --lovasz-weight; lovasz_weight == 0 never reaches a Lovasz op.  The kernels: test_lovasz_gpu.py."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lovasz_reference as R

from test_dice_loss_gpu import CE_CASES           # the shapes only: that module's tests are GPU-marked as a whole


@pytest.fixture(scope='module')
def lib():
    from segland_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


# --------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_binned_loss_is_within_half_a_bin_of_the_sorted_loss(K, hw, HW):
    """|binned - exact_sorted| <= 1 / (2 NB): the Lovasz extension of a class's Jaccard loss is 1-Lipschitz in the sup norm and a bin centre is at most 1 / (2 NB) from
    every error of its bin"""
    r = R.case(K, hw, HW)
    print('K %d %s -> %s: binned %.8g, sorted %.8g, difference %.3g (bound %.3g), %d present classes, %d valid pixels'
          % (K, hw, HW, r['loss'], r['exact'], abs(r['loss'] - r['exact']), 0.5 / R.NB, r['n_present'], r['n_valid']))
    assert r['exact'] > 0.1
    assert abs(r['loss'] - r['exact']) <= 0.5 / R.NB


@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_histograms_count_every_valid_pixel_once_per_class(K, hw, HW):
    r = R.case(K, hw, HW)
    t = r['target']
    assert r['hist'].sum((1, 2)).tolist() == [r['n_valid']] * K
    assert r['hist'][:, :, 0].sum(1).tolist() == [int((t == c).sum()) for c in range(K)]
    # an absent class has a zero row, an empty bin a zero entry, and the rows of the present classes are non-negative (dJ >= 0: J grows as the walk goes down)
    absent = r['hist'][:, :, 0].sum(1) == 0
    assert not r['table'][absent].any() and not r['table'][r['hist'].sum(2) == 0].any() and bool((r['table'] >= 0).all())
    if HW == (8, 8):
        assert r['n_present'] == 7                        # one 8 x 8 block map: a class absent from the batch


def test_closed_form_gradient_is_the_autograd_gradient_of_the_binned_loss():
    """with the table held constant the subgradient is that of S(e) = sum_i sum_c tab[c][bin(e_ic)] e_ic, linear in the errors; its float64 autograd gradient through
    softmax and F.interpolate equals grad(), the header's closed form p_k (q_k - sum_c p_c q_c) pushed through the transposed upsample"""
    K, hw, HW = CE_CASES[1]
    r = R.case(K, hw, HW)
    pr = r['preds'].double().clone().requires_grad_(True)
    e, fg, _ = R.errors(R.upsample(pr, r['target']), r['target'])
    w = r['table'][torch.arange(K)[None, :], R.bins_of(e.detach())]
    # d e / d p is -1 for the label's own error (e = 1 - p_t) and +1 elsewhere: the sign of q
    (w * e).sum().backward()
    np.testing.assert_allclose(pr.grad.numpy(), r['grad'].numpy(), rtol=1e-9, atol=1e-15)
    assert float(r['grad'].abs().max()) > 1e-6


@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_inputs_keep_the_bin_edge_slack_small(K, hw, HW):
    """Conditions on the inputs, from the reference alone, so that the GPU tests cannot hide behind their slack: the margin m (8 x float32-vs-float64 of e) is below the
    4e-6 the shares were first measured with, at most 2 % of the (pixel, class) pairs lie within m of a bin edge, and the slack is at most 5 % of max |grad|"""
    r = R.case(K, hw, HW)
    share = r['near_edge'] / r['pairs']
    worst = float(r['slack'].max()) / float(r['grad'].abs().max())
    print('K %d %s -> %s: margin %.3g, near-edge pairs %d of %d (%.3f %%), max slack %.3g = %.2f %% of max |grad| %.3g'
          % (K, hw, HW, r['m'], r['near_edge'], r['pairs'], 100 * share, float(r['slack'].max()), 100 * worst, float(r['grad'].abs().max())))
    assert 0 < r['m'] <= 4e-6
    assert share <= 0.02
    assert worst <= 0.05
    assert bool((r['slack'] >= 0).all())


# --------------------------------------------------------------------------------------------- the library
ENTRIES = ('sl_lovasz_bins', 'sl_lovasz_workspace', 'sl_upsample_lovasz_hist', 'sl_lovasz_scan', 'sl_upsample_lovasz_bwd')


def test_lovasz_entries_are_exported_and_declared(lib):
    from segland_amd import _lib
    decl = _lib.declared_functions()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in decl, name
    assert [len(decl[n][1]) for n in ENTRIES] == [0, 1, 12, 5, 18]
    assert decl['sl_lovasz_workspace'][0] is C.c_size_t
    assert lib.sl_lovasz_bins() == R.NB
    assert [lib.sl_lovasz_workspace(K) for K in (0, 1, 8, 33, 34)] == [0, R.NB * 8 + 16, 8 * (R.NB * 8 + 16), 33 * (R.NB * 8 + 16), 0]
    # no existing signature gained an argument
    assert len(decl['sl_upsample_ce_bwd'][1]) == 13 and len(decl['sl_upsample_ce_dice_bwd'][1]) == 16 and len(decl['sl_upsample_focal_dice_bwd'][1]) == 17


def test_lovasz_entries_validate_before_any_launch(lib):
    """SL_EINVAL (-1) with a message and no launch (the pointers are not device memory: a launch would fault)"""
    d = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string().decode()
    big = lib.sl_lovasz_workspace(33)
    hist = lambda K=8, lg=d, t=d, ws=d, n=big, B=2, H=64: lib.sl_upsample_lovasz_hist(lg, t, B, K, 8, 8, H, 64, 255, ws, n, None)
    assert hist(K=34) == -1 and '34 logit channels' in err() and 'at most 33' in err()
    assert hist(K=0) == -1 and 'at most 33' in err()
    assert hist(H=0) == -1 and 'bad shape' in err()
    assert hist(B=1 << 16, H=1 << 10) == -1 and '2^32' in err()          # 2^16 * 2^10 * 64 = 2^32 pixels
    assert hist(n=lib.sl_lovasz_workspace(8) - 1) == -1 and 'workspace' in err()
    for buf in ('lg', 't', 'ws'):
        assert hist(**{buf: None}) == -1 and 'null' in err(), buf
    scan = lambda K=8, ws=d, out=d, tab=d: lib.sl_lovasz_scan(ws, K, out, tab, None)
    assert scan(K=34) == -1 and 'at most 33' in err()
    for buf in ('ws', 'out', 'tab'):
        assert scan(**{buf: None}) == -1 and 'null' in err(), buf
    bwd = lambda gamma=0.0, K=8, eps=0.0, lg=d, t=d, lo=d, coef=None, tab=d, gs=d, out=d, H=64: lib.sl_upsample_lovasz_bwd(lg, t, None, eps, gamma, lo, coef, tab, gs, 2, K, 8, 8,
                                                                                                                        H, 64, 255, out, None)
    assert bwd(gamma=0.5) == -1 and 'gamma 0.5' in err()
    assert bwd(gamma=float('nan')) == -1 and 'gamma nan' in err()
    assert bwd(gamma=float('inf')) == -1 and 'gamma inf' in err()
    assert bwd(K=34) == -1 and '34 logit channels' in err()
    assert bwd(eps=1.5) == -1 and 'label_smoothing' in err()
    assert bwd(H=0) == -1 and 'bad shape' in err()
    for buf in ('lg', 't', 'lo', 'tab', 'gs', 'out'):
        assert bwd(**{buf: None}) == -1 and 'null' in err(), buf


# --------------------------------------------------------------------------------------------- criterion and drivers
def test_orth_loss_keeps_lovasz_weight_as_a_plain_float():
    from segland_amd.loss.criterion import OrthLoss
    assert OrthLoss(255).lovasz_weight == 0.0
    crit = OrthLoss(255, weight=[1.0, 0.5, 2.0], dice_weight=0.5, focal_gamma=2, lovasz_weight=1)
    assert type(crit.lovasz_weight) is float and crit.lovasz_weight == 1.0
    assert [n for n, _ in crit.named_buffers()] == ['weight'] and not list(crit.parameters()) and len(crit.state_dict()) == 0
    for bad in (-1.0, -1e-9, float('inf'), float('-inf'), float('nan')):
        with pytest.raises(ValueError, match='lovasz_weight'):
            OrthLoss(255, lovasz_weight=bad)


def test_get_loss_with_and_without_the_field():
    from segland_amd.loss import get_loss
    assert get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255)).lovasz_weight == 0.0
    new = get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, dice_weight=0.5, lovasz_weight=0.75))
    assert new.lovasz_weight == 0.75 and new.dice_weight == 0.5
    with pytest.raises(ValueError):
        get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, lovasz_weight=-0.5))


@pytest.mark.parametrize('ft', [False, True])
def test_parsers_carry_the_lovasz_weight_to_the_criterion(ft, capsys):
    """train_base (ft False) and ft_pop (ft True) build their parser with drivers.build_parser and their criterion with loss.get_loss"""
    from segland_amd.drivers import build_parser
    from segland_amd.loss import get_loss
    p = build_parser(ft)
    assert p.parse_args([]).lovasz_weight == 0.0
    a = p.parse_args(['--lovasz-weight', '0.5', '--dice-weight', '0.25', '--model', 'pspnet_pop'])
    assert a.lovasz_weight == 0.5
    a.ignore_label = 255
    crit = get_loss(a)
    assert crit.lovasz_weight == 0.5 and crit.dice_weight == 0.25
    for bad in ('-1', 'nan', 'inf', 'x'):
        with pytest.raises(SystemExit):
            p.parse_args(['--lovasz-weight', bad])
    capsys.readouterr()


@pytest.mark.parametrize('module', ['train_base', 'ft_pop'])
def test_both_drivers_use_the_common_parser_and_get_loss(module):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'segland_amd', module + '.py')).read()
    assert 'build_parser(' in src and 'get_loss(' in src


def test_the_log_line_names_the_lovasz_weight_only_where_it_is_on(caplog):
    import logging
    from segland_amd.drivers import build_parser, log_loss_options
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        log_loss_options(build_parser(False).parse_args(['--dice-weight', '0.5', '--lovasz-weight', '0.75', '--ohem-thresh', '0.7']))
        log_loss_options(build_parser(True).parse_args(['--label-smoothing', '0.1']))
    assert [r.getMessage() for r in caplog.records] == [
        'segmentation loss: class weights none, label smoothing 0, dice weight 0.5, lovasz weight 0.75, hard-pixel mining: threshold 0.7, at least 100000 pixels per batch',
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

    def lov_fwd(logits, target, ignore_index, *a, **kw):
        seen.append('upsample_lovasz_fwd')
        return torch.zeros(2), torch.zeros(logits.shape[1], R.NB)
    monkeypatch.setattr(ops, 'upsample_lovasz_fwd', lov_fwd)
    monkeypatch.setattr(ops, 'upsample_lovasz_bwd', bwd('upsample_lovasz_bwd'))
    return seen


def _one_step(crit):
    preds = torch.zeros(2, 8, 4, 4, requires_grad=True)
    d = crit(preds, torch.zeros(2, 16, 16, dtype=torch.int64), proto_sim=torch.ones(3, 3), aux_preds=torch.zeros(2, 8, 4, 4, requires_grad=True))
    d['total_loss'].backward()
    return d


def test_lovasz_weight_zero_never_reaches_a_lovasz_op(calls, monkeypatch):
    """lovasz_weight == 0 calls exactly the functions it called before: with the two Lovasz ops patched to raise, every criterion without the term still runs on its ops"""
    from segland_amd import ops
    from segland_amd.loss.criterion import OrthLoss

    def boom(*a, **kw):
        raise AssertionError('a Lovasz op was reached with lovasz_weight == 0')
    monkeypatch.setattr(ops, 'upsample_lovasz_fwd', boom)
    monkeypatch.setattr(ops, 'upsample_lovasz_bwd', boom)
    assert list(_one_step(OrthLoss(255, lovasz_weight=0.0))) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss']
    assert sorted(calls) == ['upsample_ce_bwd'] * 2 + ['upsample_ce_fwd'] * 2
    del calls[:]
    assert list(_one_step(OrthLoss(255, dice_weight=0.5, focal_gamma=2.0, lovasz_weight=0))) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss', 'dice_loss']
    assert sorted(calls) == ['upsample_focal_dice_bwd'] * 2 + ['upsample_focal_dice_fwd'] * 2


@pytest.mark.parametrize('dice,gamma,fwd', [(0.0, 0.0, 'upsample_ce_fwd'), (0.5, 0.0, 'upsample_ce_dice_fwd'), (0.0, 2.0, 'upsample_focal_fwd'), (0.5, 2.0, 'upsample_focal_dice_fwd')])
def test_lovasz_weight_routes_both_heads_to_one_backward_launch(calls, dice, gamma, fwd):
    """the forward of the chosen cross-entropy / Dice form, untouched, plus the Lovasz forward; the backward is the Lovasz op alone, once per head"""
    from segland_amd.loss.criterion import OrthLoss
    d = _one_step(OrthLoss(255, dice_weight=dice, focal_gamma=gamma, lovasz_weight=0.5))
    assert list(d) == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss'] + (['dice_loss'] if dice else []) + ['lovasz_loss']
    assert calls[:4] == [fwd, 'upsample_lovasz_fwd'] * 2 and calls[4:] == ['upsample_lovasz_bwd'] * 2
