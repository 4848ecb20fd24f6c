"""Class weights and label smoothing of the fused upsample + cross-entropy loss, CPU side: the two weighted entry points exist and validate before any launch, OrthLoss
keeps its weights out of every state_dict, get_loss and both drivers' parsers carry the two controls.  The kernels themselves: test_weighted_ce_gpu.py."""
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


def test_weighted_entries_are_exported_and_declared(lib):
    from segland_amd import _lib
    assert hasattr(lib, 'sl_upsample_ce_weighted_fwd') and hasattr(lib, 'sl_upsample_ce_weighted_bwd')
    decl = _lib.declared_functions()
    assert decl['sl_upsample_ce_weighted_fwd'][1][3] is C.c_float and len(decl['sl_upsample_ce_weighted_fwd'][1]) == 13
    assert decl['sl_upsample_ce_weighted_bwd'][1][3] is C.c_float and len(decl['sl_upsample_ce_weighted_bwd'][1]) == 15


def test_weighted_entries_validate_before_any_launch(lib):
    d = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string().decode()
    fwd = lambda w, eps, K: lib.sl_upsample_ce_weighted_fwd(d, d, w, eps, 2, K, 8, 8, 64, 64, 255, d, None)
    bwd = lambda w, eps, K: lib.sl_upsample_ce_weighted_bwd(d, d, w, eps, d, d, 2, K, 8, 8, 64, 64, 255, d, None)
    for call in (fwd, bwd):
        assert call(d, 0.1, 34) == -1 and '34 logit channels' in err() and 'at most 33' in err()
        assert call(d, 0.1, 0) == -1 and 'at most 33' in err()
        assert call(d, 1.5, 8) == -1 and 'label_smoothing' in err()
        assert call(d, -0.1, 8) == -1 and 'label_smoothing' in err()
        assert call(d, float('nan'), 8) == -1 and 'label_smoothing' in err()
        assert call(None, 0.1, 8) == -1 and 'class_weight' in err()
    # the plain pair keeps its own checks
    assert lib.sl_upsample_ce_fwd(d, d, 2, 34, 8, 8, 64, 64, 255, d, None) == -1 and 'at most 33' in err()
    assert lib.sl_upsample_ce_bwd(d, d, d, d, 2, 34, 8, 8, 64, 64, 255, d, None) == -1 and 'at most 33' in err()


def test_orth_loss_keeps_weights_out_of_the_state_dict():
    from segland_amd.loss.criterion import OrthLoss
    plain = OrthLoss(255)
    crit = OrthLoss(255, weight=[1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.75, 1.25], label_smoothing=0.1)
    assert len(plain.state_dict()) == 0 and len(crit.state_dict()) == 0
    assert plain.weight is None and plain.label_smoothing == 0.0
    assert crit.weight.dtype == torch.float32 and tuple(crit.weight.shape) == (8,) and crit.label_smoothing == 0.1
    assert [n for n, _ in crit.named_buffers()] == ['weight'] and not list(crit.parameters())
    assert OrthLoss(255, weight=[1.0, 2.0]).to(torch.float64).weight.dtype == torch.float64      # a buffer: it follows .to()
    src = torch.tensor([1.0, 2.0], dtype=torch.float64)
    c2 = OrthLoss(255, weight=src)
    src[0] = 5.0
    assert c2.weight.dtype == torch.float32 and c2.weight.tolist() == [1.0, 2.0]  # its own float32 copy
    with pytest.raises(ValueError):
        OrthLoss(255, reduction='sum', weight=[1.0, 2.0])
    with pytest.raises(ValueError):
        OrthLoss(255, label_smoothing=1.5)
    with pytest.raises(ValueError):
        OrthLoss(255, weight=[[1.0, 2.0]])
    # a model holding the weighted criterion has the pinned key count of the plain one
    from segland_amd.networks.pspnet_pop import GFSS_Model
    keys = lambda c: set(GFSS_Model(n_base=7, criterion=c, backbone='resnet50', pretrained_model=None, dilated=True, os=8).state_dict())
    assert keys(crit) == keys(plain) == keys(None)


def test_wrong_weight_length_names_both_numbers():
    from segland_amd.loss.criterion import OrthLoss
    crit = OrthLoss(255, weight=[1.0] * 7)
    with pytest.raises(ValueError, match=r'7 class weights for 8 logit channels'):
        crit.seg_loss(torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 16, dtype=torch.int64))


def test_get_loss_with_and_without_the_new_fields():
    from segland_amd.loss import get_loss
    old = get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255))
    assert old.weight is None and old.label_smoothing == 0.0 and old.ignore_index == 255
    new = get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, class_weights=(1.0, 2.0, 0.5), label_smoothing=0.05))
    assert new.weight.tolist() == [1.0, 2.0, 0.5] and new.label_smoothing == 0.05
    assert get_loss(argparse.Namespace(model='swin_pop', ignore_label=255, class_weights='1,2,0.5', label_smoothing=0.0)).weight.tolist() == [1.0, 2.0, 0.5]
    for empty in ('', (), None):
        assert get_loss(argparse.Namespace(model='pspnet_pop', ignore_label=255, class_weights=empty, label_smoothing=0.0)).weight is None
    with pytest.raises(RuntimeError):
        get_loss(argparse.Namespace(model='pspnet', ignore_label=255, class_weights=(1.0,), label_smoothing=0.1))


@pytest.mark.parametrize('ft', [False, True])
def test_parsers_accept_the_two_flags(ft, capsys):
    from segland_amd.drivers import build_parser
    from segland_amd.loss import get_loss
    p = build_parser(ft)
    a = p.parse_args([])
    assert a.class_weights == () and a.label_smoothing == 0.0
    a = p.parse_args(['--class-weights', '1,0.5, 2,0', '--label-smoothing', '0.1', '--model', 'pspnet_pop'])
    assert a.class_weights == (1.0, 0.5, 2.0, 0.0) and a.label_smoothing == 0.1
    a.ignore_label = 255
    crit = get_loss(a)
    assert crit.weight.tolist() == [1.0, 0.5, 2.0, 0.0] and crit.label_smoothing == 0.1
    for bad in (['--class-weights', '1,two,3'], ['--class-weights', '1,,3'], ['--class-weights', '1,-2'], ['--class-weights', '1,nan'],
                ['--label-smoothing', '1.5'], ['--label-smoothing', 'much']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    capsys.readouterr()


def test_loss_options_are_logged_once(caplog):
    import logging
    from segland_amd.drivers import build_parser, log_loss_options
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        log_loss_options(build_parser(False).parse_args(['--class-weights', '1,0.5', '--label-smoothing', '0.1']))
        log_loss_options(argparse.Namespace())
    assert [r.getMessage() for r in caplog.records] == ['segmentation loss: class weights 1,0.5, label smoothing 0.1',
                                                        'segmentation loss: class weights none, label smoothing 0']
