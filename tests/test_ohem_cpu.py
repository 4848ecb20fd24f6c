"""Online hard-pixel mining (OHEM), CPU side: the four entry points exist, are declared and validate before any launch; both drivers' parsers carry --ohem-thresh and
--ohem-min-kept; OrthLoss keeps them as plain Python values and refuses bad ones; get_loss wires them, also from a namespace without the fields; with mining off the op is
never called, with mining on each head's criterion runs on that head's mined map; the torch restatement of the definition (tests/ohem_reference.py) gives a hand-computed
2 x 2 case.  The kernels themselves: test_ohem_gpu.py."""
import argparse
import ctypes as C
import math
import os

import pytest
import torch

import ohem_reference as R


@pytest.fixture(scope='module')
def lib():
    from segland_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_entries_are_exported_and_declared(lib):
    from segland_amd import _lib
    decl = _lib.declared_functions()
    for name in ('sl_upsample_ohem_prob', 'sl_ohem_workspace', 'sl_ohem_threshold', 'sl_ohem_mine'):
        assert hasattr(lib, name) and name in decl, name
    assert len(decl['sl_upsample_ohem_prob'][1]) == 11
    assert decl['sl_ohem_workspace'] == (C.c_size_t, [C.c_int] * 3)
    assert decl['sl_ohem_threshold'][1][1:4] == [C.c_longlong, C.c_float, C.c_longlong] and decl['sl_ohem_threshold'][1][5] is C.c_size_t and len(decl['sl_ohem_threshold'][1]) == 9
    assert len(decl['sl_ohem_mine'][1]) == 8
    # the loss entry points keep their signatures
    assert len(decl['sl_upsample_ce_fwd'][1]) == 11 and len(decl['sl_upsample_ce_bwd'][1]) == 13 and len(decl['sl_upsample_ce_dice_fwd'][1]) == 13


def test_entries_validate_before_any_launch(lib):
    d = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string().decode()
    need = lib.sl_ohem_workspace(2, 64, 64)
    assert need > 0 and lib.sl_ohem_workspace(2, 0, 64) == 0
    prob = lambda K, lg=d, tg=d, out=d: lib.sl_upsample_ohem_prob(lg, tg, 2, K, 8, 8, 64, 64, 255, out, None)
    assert prob(34) == -1 and '34 logit channels' in err() and 'at most 33' in err()
    assert prob(0) == -1 and 'at most 33' in err()
    for kw in (dict(lg=None), dict(tg=None), dict(out=None)):
        assert prob(8, **kw) == -1 and 'null' in err()
    thr = lambda thresh=0.7, min_kept=10, n=8192, p=d, ws=d, nbytes=need, theta=d, counts=d: lib.sl_ohem_threshold(p, n, thresh, min_kept, ws, nbytes, theta, counts, None)
    for bad in (0.0, -0.1, 1.5, float('nan')):
        assert thr(thresh=bad) == -1 and 'thresh' in err() and '(0, 1]' in err(), bad
    assert thr(min_kept=0) == -1 and 'min_kept 0' in err()
    assert thr(min_kept=-5) == -1 and 'min_kept' in err()
    assert thr(n=0) == -1 and thr(n=1 << 31) == -1 and 'pixels' in err()
    assert thr(nbytes=need - 1) == -1 and 'workspace %d < %d' % (need - 1, need) in err()
    for kw in (dict(p=None), dict(ws=None), dict(theta=None), dict(counts=None)):
        assert thr(**kw) == -1 and 'null' in err()
    mine = lambda n=8192, p=d, tg=d, theta=d, counts=d, out=d: lib.sl_ohem_mine(p, tg, theta, counts, n, 255, out, None)
    assert mine(n=0) == -1 and 'pixels' in err()
    for kw in (dict(p=None), dict(tg=None), dict(theta=None), dict(counts=None), dict(out=None)):
        assert mine(**kw) == -1 and 'null' in err()


@pytest.mark.parametrize('ft', [False, True])
def test_parsers_carry_the_mining_flags(ft, capsys):
    from segland_amd.drivers import build_parser
    from segland_amd.loss import get_loss
    p = build_parser(ft)
    a = p.parse_args(['--model', 'pspnet_pop'])
    assert a.ohem_thresh == 0.0 and a.ohem_min_kept == 100000
    a.ignore_label = 255
    assert get_loss(a).ohem_thresh is None                                  # 0 from the command line is off
    a = p.parse_args(['--ohem-thresh', '0.7', '--ohem-min-kept', '5000', '--model', 'pspnet_pop'])
    assert a.ohem_thresh == 0.7 and a.ohem_min_kept == 5000 and type(a.ohem_min_kept) is int
    a.ignore_label = 255
    crit = get_loss(a)
    assert crit.ohem_thresh == 0.7 and crit.ohem_min_kept == 5000
    assert p.parse_args(['--ohem-thresh', '1']).ohem_thresh == 1.0
    for bad in ('-0.1', '1.5', 'nan', 'x'):
        with pytest.raises(SystemExit):
            p.parse_args(['--ohem-thresh', bad])
    for bad in ('0', '-3', '2.5', 'x'):
        with pytest.raises(SystemExit):
            p.parse_args(['--ohem-min-kept', bad])
    capsys.readouterr()


def test_the_log_line_names_the_mining_controls_only_where_they_are_on(caplog):
    import logging
    from segland_amd.drivers import build_parser, log_loss_options
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        log_loss_options(build_parser(False).parse_args(['--ohem-thresh', '0.7', '--ohem-min-kept', '5000']))
        log_loss_options(build_parser(True).parse_args(['--dice-weight', '0.5', '--ohem-thresh', '0.9']))
        log_loss_options(build_parser(False).parse_args(['--ohem-min-kept', '5000']))
        log_loss_options(argparse.Namespace())
    assert [r.getMessage() for r in caplog.records] == ['segmentation loss: class weights none, label smoothing 0, hard-pixel mining: threshold 0.7, at least 5000 pixels per batch',
                                                        'segmentation loss: class weights none, label smoothing 0, dice weight 0.5, hard-pixel mining: threshold 0.9, at least 100000 pixels per batch',
                                                        'segmentation loss: class weights none, label smoothing 0',
                                                        'segmentation loss: class weights none, label smoothing 0']


def test_orth_loss_keeps_the_mining_controls_as_plain_values():
    from segland_amd.loss.criterion import OrthLoss
    plain = OrthLoss(255)
    assert plain.ohem_thresh is None and plain.ohem_min_kept == 100000
    assert OrthLoss(255, ohem_thresh=0).ohem_thresh is None and OrthLoss(255, ohem_thresh=0.0, ohem_min_kept=7).ohem_thresh is None
    crit = OrthLoss(255, weight=[1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.75, 1.25], dice_weight=0.5, ohem_thresh=0.7, ohem_min_kept=5000)
    assert type(crit.ohem_thresh) is float and crit.ohem_thresh == 0.7 and type(crit.ohem_min_kept) is int and crit.ohem_min_kept == 5000
    assert OrthLoss(255, ohem_thresh=1).ohem_thresh == 1.0
    assert [n for n, _ in crit.named_buffers()] == ['weight'] and not list(crit.parameters()) and len(crit.state_dict()) == 0
    assert len(OrthLoss(255, ohem_thresh=0.7).state_dict()) == 0
    for bad in (dict(ohem_thresh=-0.1), dict(ohem_thresh=1.5), dict(ohem_thresh=float('nan')), dict(ohem_thresh=float('inf')), dict(ohem_thresh=0.7, ohem_min_kept=0),
                dict(ohem_min_kept=0), dict(ohem_min_kept=-1), dict(ohem_min_kept=2.5), dict(ohem_min_kept=True)):
        with pytest.raises(ValueError):
            OrthLoss(255, **bad)
    from segland_amd.networks.pspnet_pop import GFSS_Model
    keys = lambda c: set(GFSS_Model(n_base=7, criterion=c, backbone='resnet50', pretrained_model=None, dilated=True, os=8).state_dict())
    assert keys(crit) == keys(plain)


def test_get_loss_with_and_without_the_fields():
    from segland_amd.loss import get_loss
    old = get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255))
    assert old.ohem_thresh is None and old.ohem_min_kept == 100000 and old.dice_weight == 0.0 and old.weight is None
    new = get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, ohem_thresh=0.7, ohem_min_kept=123, dice_weight=0.5))
    assert new.ohem_thresh == 0.7 and new.ohem_min_kept == 123 and new.dice_weight == 0.5
    assert get_loss(argparse.Namespace(model='swin_pop', ignore_label=255, ohem_thresh=0.5)).ohem_min_kept == 100000
    with pytest.raises(ValueError):
        get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, ohem_thresh=1.5))
    with pytest.raises(ValueError):
        get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, ohem_thresh=0.7, ohem_min_kept=0))


class _Fn:
    """stands in for the fused autograd functions on the CPU: records the label map it is handed"""

    def __init__(self, n_out):
        self.n_out, self.targets = n_out, []

    def apply(self, preds, target, *rest):
        self.targets.append(target)
        out = preds.sum() * 0.0 + 1.0
        return out if self.n_out == 1 else (out, out * 2.0)


def test_off_never_calls_the_op_and_on_hands_each_head_its_own_mined_map(monkeypatch):
    from segland_amd import ops
    from segland_amd.loss import criterion
    ce, hyb = _Fn(1), _Fn(2)
    monkeypatch.setattr(criterion, 'UpsampleCEFn', ce)
    monkeypatch.setattr(criterion, 'UpsampleCEDiceFn', hyb)

    def boom(*a, **k):
        raise AssertionError('ops.ohem_mine called with mining off')
    monkeypatch.setattr(ops, 'ohem_mine', boom)
    preds, aux = torch.zeros(2, 8, 4, 4), torch.ones(2, 8, 6, 6)
    target = torch.zeros(2, 16, 16, dtype=torch.int64)
    sim = torch.eye(4)
    for crit in (criterion.OrthLoss(255), criterion.OrthLoss(255, ohem_thresh=None), criterion.OrthLoss(255, ohem_thresh=0), criterion.OrthLoss(255, dice_weight=0.5)):
        d = crit(preds, target, proto_sim=sim, aux_preds=aux)
        assert 'ohem_frac' not in d and list(d)[:4] == ['total_loss', 'seg_loss', 'aux_loss', 'orth_loss']
    assert all(t is target for t in ce.targets + hyb.targets) and len(ce.targets) == 6 and len(hyb.targets) == 2

    calls = []

    def fake_mine(logits, tgt, ignore_index, thresh, min_kept):
        assert not logits.requires_grad and not torch.is_grad_enabled()
        calls.append((tuple(logits.shape), tgt, ignore_index, thresh, min_kept))
        return torch.full_like(tgt, len(calls)), torch.tensor([thresh]), torch.tensor([200, 50, 50 * len(calls)])
    monkeypatch.setattr(ops, 'ohem_mine', fake_mine)
    ce.targets.clear(), hyb.targets.clear()
    for crit, fn in ((criterion.OrthLoss(255, ohem_thresh=0.7, ohem_min_kept=50), ce), (criterion.OrthLoss(255, dice_weight=0.5, ohem_thresh=0.7, ohem_min_kept=50), hyb)):
        calls.clear()
        d = crit(preds.clone().requires_grad_(True), target, proto_sim=sim, aux_preds=aux)
        assert [c[0] for c in calls] == [(2, 8, 4, 4), (2, 8, 6, 6)] and all(c[1] is target and c[2:] == (255, 0.7, 50) for c in calls)
        assert [int(t[0, 0, 0]) for t in fn.targets] == [1, 2], 'each head runs on its own mined map'
        assert list(d)[-1] == 'ohem_frac' and float(d['ohem_frac']) == 0.25 and not d['ohem_frac'].requires_grad          # the main head's n_kept / n
        fn.targets.clear()
    assert bool((target == 0).all())


def test_reference_on_a_hand_computed_case():
    """2 x 2 pixels at the identity scale, two channels: p of the true class is the logistic function of the logit difference: 1/4, 1/2, 3/4, 9/10"""
    l3, l9 = math.log(3.0), math.log(9.0)
    logits = torch.tensor([[[[0.0, 1.0], [l3, l9]], [[l3, 1.0], [0.0, 0.0]]]])            # channel 0, channel 1
    target = torch.tensor([[[0, 1], [0, 0]]])
    p, valid = R.true_class_prob(logits, target)
    assert bool(valid.all()) and torch.allclose(p, torch.tensor([[[0.25, 0.5], [0.75, 0.9]]]), rtol=1e-6)
    r = R.mine(logits, target, 0.3, 2)                                                   # q = 0.5 > thresh: min_kept decides
    assert (r['n'], r['k'], r['n_kept'], r['binds'], r['ties']) == (4, 2, 2, True, 1) and abs(r['theta'] - 0.5) < 1e-6
    assert r['mined'].tolist() == [[[0, 1], [255, 255]]] and abs(r['gap'] - 0.25) < 1e-6
    loss, dice, _ = R.head_loss(logits, target, 0.3, 2)
    assert dice is None and abs(float(loss) - (math.log(4.0) + math.log(2.0)) / 2) < 1e-6
    r = R.mine(logits, target, 0.8, 1)                                                   # q = 0.25 <= thresh: the threshold decides
    assert (r['k'], r['n_kept'], r['binds']) == (1, 3, False) and r['mined'].tolist() == [[[0, 1], [0, 255]]] and abs(r['theta'] - 0.8) < 1e-6 and abs(r['gap'] - 0.05) < 1e-6
    assert R.mine(logits, target, 0.3, 100)['mined'].tolist() == target.tolist()         # min_kept >= n keeps everything
    t2 = torch.tensor([[[255, 1], [0, 7]]])                                              # an ignored and an out-of-range label: n = 2
    r = R.mine(logits, t2, 0.6, 1)
    assert (r['n'], r['k'], r['n_kept']) == (2, 1, 1) and r['mined'].tolist() == [[[255, 1], [255, 255]]] and r['p'][0, 0, 0] == 2.0 and r['p'][0, 1, 1] == 2.0
    r = R.mine(logits, torch.full_like(target, 255), 0.6, 1)
    assert r['n'] == 0 and r['mined'].tolist() == [[[255, 255], [255, 255]]] and r['n_kept'] == 0
    # ties: two pixels share p = 1/2 exactly; min_kept = 1 keeps both
    lg = torch.zeros(1, 2, 1, 2)
    r = R.mine(lg, torch.tensor([[[0, 1]]]), 0.1, 1)
    assert r['ties'] == 2 and r['n_kept'] == 2 and r['binds']
