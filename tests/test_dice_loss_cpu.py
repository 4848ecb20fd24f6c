"""Hybrid cross-entropy + soft Dice criterion, CPU side: the four sl_upsample_ce_dice_* entry points exist, are declared and validate before any launch; OrthLoss keeps
dice_weight / dice_smooth as plain floats (no buffer, no state_dict key) and refuses bad values; get_loss and both drivers' parsers carry --dice-weight; the log line names
the Dice weight only where it is on.  The kernels themselves: test_dice_loss_gpu.py."""
import argparse
import ctypes as C
import os

import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    from segland_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


ENTRIES = ('sl_upsample_ce_dice_rows', 'sl_upsample_ce_dice_fwd', 'sl_upsample_ce_dice_finalize', 'sl_upsample_ce_dice_bwd')


def test_dice_entries_are_exported_and_declared(lib):
    from segland_amd import _lib
    decl = _lib.declared_functions()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in decl, name
    assert len(decl['sl_upsample_ce_dice_rows'][1]) == 3
    assert decl['sl_upsample_ce_dice_fwd'][1][3] is C.c_float and len(decl['sl_upsample_ce_dice_fwd'][1]) == 13
    assert decl['sl_upsample_ce_dice_finalize'][1][2] is C.c_float and len(decl['sl_upsample_ce_dice_finalize'][1]) == 10
    assert decl['sl_upsample_ce_dice_bwd'][1][3] is C.c_float and len(decl['sl_upsample_ce_dice_bwd'][1]) == 16
    # the plain and the weighted pairs keep their signatures
    assert len(decl['sl_upsample_ce_fwd'][1]) == 11 and len(decl['sl_upsample_ce_bwd'][1]) == 13
    assert len(decl['sl_upsample_ce_weighted_fwd'][1]) == 13 and len(decl['sl_upsample_ce_weighted_bwd'][1]) == 15


def test_partial_rows_never_mix_samples(lib):
    """the row count is a multiple of B (rows / B blocks per sample), one row for a map of up to 256 pixels, about 1024 rows in all at the bench shape"""
    assert lib.sl_upsample_ce_dice_rows(2, 8, 8) == 2
    assert lib.sl_upsample_ce_dice_rows(2, 40, 33) == 2 * 6
    assert lib.sl_upsample_ce_dice_rows(16, 512, 512) == 1024
    assert lib.sl_upsample_ce_dice_rows(3, 512, 512) == 3 * 341
    assert lib.sl_upsample_ce_dice_rows(5000, 64, 64) == 5000


def test_dice_entries_validate_before_any_launch(lib):
    d = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string().decode()
    fwd = lambda eps, K, lg=d, part=d: lib.sl_upsample_ce_dice_fwd(lg, d, None, eps, 2, K, 8, 8, 64, 64, 255, part, None)
    bwd = lambda eps, K, coef=d, gs=d: lib.sl_upsample_ce_dice_bwd(d, d, None, eps, d, coef, gs, 2, K, 8, 8, 64, 64, 255, d, None)
    fin = lambda smooth, K, part=d, out=d, coef=d: lib.sl_upsample_ce_dice_finalize(part, None, smooth, 2, K, 64, 64, out, coef, None)
    for call in (fwd, bwd):
        assert call(0.1, 34) == -1 and '34 logit channels' in err() and 'at most 33' in err()
        assert call(0.1, 0) == -1 and 'at most 33' in err()
        assert call(1.5, 8) == -1 and 'label_smoothing' in err()
        assert call(-0.1, 8) == -1 and 'label_smoothing' in err()
        assert call(float('nan'), 8) == -1 and 'label_smoothing' in err()
    assert fwd(0.0, 8, lg=None) == -1 and 'null' in err()
    assert fwd(0.0, 8, part=None) == -1 and 'null' in err()
    assert bwd(0.0, 8, coef=None) == -1 and 'null' in err()
    assert bwd(0.0, 8, gs=None) == -1 and 'null' in err()
    assert fin(1.0, 34) == -1 and '34 logit channels' in err() and 'at most 33' in err()
    assert fin(1.0, 0) == -1 and 'at most 33' in err()
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert fin(bad, 8) == -1 and 'smooth' in err(), bad
    assert fin(1.0, 8, part=None) == -1 and 'null' in err()
    assert fin(1.0, 8, out=None) == -1 and 'null' in err()
    assert fin(1.0, 8, coef=None) == -1 and 'null' in err()


def test_orth_loss_keeps_the_dice_controls_as_plain_floats():
    from segland_amd.loss.criterion import OrthLoss
    plain = OrthLoss(255)
    assert plain.dice_weight == 0.0 and plain.dice_smooth == 1.0
    crit = OrthLoss(255, weight=[1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.75, 1.25], label_smoothing=0.1, dice_weight=0.5, dice_smooth=2.0)
    assert type(crit.dice_weight) is float and crit.dice_weight == 0.5 and type(crit.dice_smooth) is float and crit.dice_smooth == 2.0
    assert [n for n, _ in crit.named_buffers()] == ['weight'] and not list(crit.parameters()) and len(crit.state_dict()) == 0
    nod = OrthLoss(255, dice_weight=1.0)
    assert nod.weight is None and len(nod.state_dict()) == 0
    for bad in (dict(dice_weight=-0.1), dict(dice_weight=float('nan')), dict(dice_weight=float('inf')), dict(dice_smooth=0.0), dict(dice_smooth=-1.0),
                dict(dice_smooth=float('nan')), dict(dice_weight=1.0, dice_smooth=float('inf'))):
        with pytest.raises(ValueError):
            OrthLoss(255, **bad)
    # a model holding the Dice criterion has the key set of the plain one
    from segland_amd.networks.pspnet_pop import GFSS_Model
    keys = lambda c: set(GFSS_Model(n_base=7, criterion=c, backbone='resnet50', pretrained_model=None, dilated=True, os=8).state_dict())
    assert keys(crit) == keys(plain) == keys(None)


def test_wrong_weight_length_is_refused_on_the_dice_path_too():
    from segland_amd.loss.criterion import OrthLoss
    crit = OrthLoss(255, weight=[1.0] * 7, dice_weight=0.5)
    with pytest.raises(ValueError, match=r'7 class weights for 8 logit channels'):
        crit.seg_loss(torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 16, dtype=torch.int64))


def test_get_loss_with_and_without_the_field():
    from segland_amd.loss import get_loss
    old = get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255))
    assert old.dice_weight == 0.0 and old.dice_smooth == 1.0 and old.weight is None
    new = get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, class_weights=(1.0, 2.0, 0.5), label_smoothing=0.05, dice_weight=0.5))
    assert new.dice_weight == 0.5 and new.weight.tolist() == [1.0, 2.0, 0.5] and new.label_smoothing == 0.05
    assert get_loss(argparse.Namespace(model='swin_pop', ignore_label=255, dice_weight=2.0)).dice_weight == 2.0
    with pytest.raises(ValueError):
        get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, dice_weight=-1.0))


@pytest.mark.parametrize('ft', [False, True])
def test_parsers_accept_the_dice_weight(ft, capsys):
    from segland_amd.drivers import build_parser
    from segland_amd.loss import get_loss
    p = build_parser(ft)
    assert p.parse_args([]).dice_weight == 0.0
    a = p.parse_args(['--dice-weight', '0.5', '--model', 'pspnet_pop'])
    assert a.dice_weight == 0.5
    a.ignore_label = 255
    assert get_loss(a).dice_weight == 0.5
    assert p.parse_args(['--dice-weight', '0']).dice_weight == 0.0
    for bad in ('-1', 'nan', 'x', 'inf'):
        with pytest.raises(SystemExit):
            p.parse_args(['--dice-weight', bad])
    capsys.readouterr()


def test_the_log_line_names_the_dice_weight_only_where_it_is_on(caplog):
    import logging
    from segland_amd.drivers import build_parser, log_loss_options
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        log_loss_options(build_parser(False).parse_args(['--class-weights', '1,0.5', '--label-smoothing', '0.1', '--dice-weight', '0.5']))
        log_loss_options(build_parser(True).parse_args(['--dice-weight', '2']))
        log_loss_options(build_parser(False).parse_args(['--class-weights', '1,0.5', '--label-smoothing', '0.1']))
        log_loss_options(argparse.Namespace())
    assert [r.getMessage() for r in caplog.records] == ['segmentation loss: class weights 1,0.5, label smoothing 0.1, dice weight 0.5',
                                                        'segmentation loss: class weights none, label smoothing 0, dice weight 2',
                                                        'segmentation loss: class weights 1,0.5, label smoothing 0.1',
                                                        'segmentation loss: class weights none, label smoothing 0']
