"""CPU-only checks of the deep-stem backbones: construction through the factory, state_dict names and shapes against the list recorded from the reference,
checkpoint round trips through load_model, the C ABI of the new stem entries (validation without a launch, launch-plan queries), and the CPU restatement
(tests/resnetv2_cpu.py) against the golden records G20 / G21 bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import golden
from oracle import formula as fm
from oracle import pop_oracle as po
import resnetv2_cpu as rv
from segland_amd import _lib


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _model(backbone='resnet50v2', **kw):
    from segland_amd.networks.pspnet_pop import GFSS_Model
    return GFSS_Model(n_base=7, criterion=None, backbone=backbone, pretrained_model=None, dilated=True, os=8, **kw)


@pytest.mark.parametrize('name,l3', [('resnet50v2', 6), ('resnet101v2', 23)])
def test_factory_builds_deep_stem(name, l3):
    from segland_amd.networks.backbones import get_backbone
    from segland_amd.networks.backbones.resnet import ResNet, ResNetv2
    net = get_backbone(nn.BatchNorm2d, backbone=name)
    assert isinstance(net, ResNetv2) and len(net.layer3) == l3
    assert tuple(net.conv1.weight.shape) == (64, 3, 3, 3) and tuple(net.conv3.weight.shape) == (128, 64, 3, 3)
    assert tuple(net.layer1[0].conv1.weight.shape) == (64, 128, 1, 1) and tuple(net.layer1[0].downsample[0].weight.shape) == (256, 128, 1, 1)
    assert isinstance(get_backbone(nn.BatchNorm2d, backbone=name[:-2]), ResNet) and not isinstance(get_backbone(nn.BatchNorm2d, backbone=name[:-2]), ResNetv2)
    with pytest.raises(RuntimeError, match='resnet50v2 / resnet101v2'):
        get_backbone(nn.BatchNorm2d, backbone='resnet18v2')


def test_state_dict_matches_the_reference_key_list():
    g = golden('g21_full_r50v2')
    sd = _model().state_dict()
    assert list(sd.keys()) == [str(k) for k in g['state_dict_keys']]
    assert ['x'.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g['state_dict_shapes']]
    assert list(rv.PopV2(n_base=7).state_dict().keys()) == list(sd.keys())


@pytest.mark.parametrize('prefix', ['', 'module.'])
def test_checkpoint_round_trip(tmp_path, prefix):
    from segland_amd.utils.pyt_utils import load_model
    ora = fm.load_formula_weights(rv.PopV2(n_base=7))
    path = str(tmp_path / 'ckpt.pth')
    torch.save({'state_dict': {prefix + k: v for k, v in ora.state_dict().items()}}, path)
    m = load_model(_model(), path, is_restore=bool(prefix))
    for (k, a), (_, b) in zip(m.state_dict().items(), ora.state_dict().items()):
        assert torch.equal(a, b), k
    # a backbone-only ImageNet checkpoint (keys conv1 / bn1 / conv2 / ...)
    torch.save({prefix + k: v for k, v in ora.backbone.state_dict().items()}, path)
    m2 = load_model(_model(), path, is_restore=bool(prefix), backbone_only=True)
    assert torch.equal(m2.backbone.conv3.weight, ora.backbone.conv3.weight) and torch.equal(m2.backbone.layer1[0].conv1.weight, ora.backbone.layer1[0].conv1.weight)


def test_late_parameters_and_groups():
    """The bucket step's cut (late = everything behind layer3) and the optimizer groups see the whole deep stem as backbone."""
    from segland_amd.utils.pyt_utils import get_parameters
    m = _model()
    late = {id(p) for p in m.late_parameters()}
    bb = m.backbone
    assert not any(id(p) in late for part in (bb.conv1, bb.bn1, bb.conv2, bb.bn2, bb.conv3, bb.bn3, bb.layer1, bb.layer3) for p in part.parameters())
    assert all(id(p) in late for p in bb.layer4.parameters()) and all(id(p) in late for p in m.decoder.parameters())
    m50 = _model('resnet50')
    late50 = {id(p) for p in m50.late_parameters()}
    assert not any(id(p) in late50 for part in (m50.backbone.conv1, m50.backbone.bn1, m50.backbone.layer3) for p in part.parameters())
    groups = get_parameters(m, lr=1e-3)
    n_bb = sum(1 for _ in bb.parameters())
    assert len(groups[0]['params']) == n_bb and sum(len(g['params']) for g in groups) == sum(1 for _ in m.parameters())


def test_new_entries_reject_bad_arguments_without_launch(lib):
    d = C.c_void_p(16)
    bf, f32 = _lib.SL_BF16, _lib.SL_F32
    assert lib.sl_stem3_conv_fwd(f32, None, d, None, None, d, None, 2, 64, 64, None, None) == -1 and b'stem3_conv_fwd' in lib.sl_last_error_string()
    assert lib.sl_stem3_conv_fwd(f32, d, d, d, None, d, None, 2, 64, 64, None, None) == -1 and b'pairs' in lib.sl_last_error_string()
    assert lib.sl_stem3_conv_fwd(f32, d, d, d, d, d, d, 2, 64, 64, None, None) == -1 and b'no statistics' in lib.sl_last_error_string()
    assert lib.sl_stem3_conv_fwd(bf, d, d, None, None, d, None, 2, 64, 64, None, None) == -1 and b'workspace' in lib.sl_last_error_string()
    assert lib.sl_stem3_conv_fwd(7, d, d, None, None, d, None, 2, 64, 64, d, None) == -1 and b'dtype' in lib.sl_last_error_string()
    assert lib.sl_stem3_conv_fwd(f32, d, d, None, None, d, None, 0, 64, 64, None, None) == -1
    need = lib.sl_stem3_conv_bwd_weight_workspace(2, 64, 64)
    assert need == 2 * 2 * 2 * 64 * 27 * 4
    assert lib.sl_stem3_conv_bwd_weight(bf, d, d, d, d, need - 1, 2, 64, 64, None) == -2 and b'workspace' in lib.sl_last_error_string()      # SL_EWORKSPACE
    assert lib.sl_stem3_conv_bwd_weight(bf, d, None, d, d, need, 2, 64, 64, None) == -1
    assert lib.sl_stem_bn_relu_pool_fwd_c(bf, d, d, d, d, None, 2, 32, 32, 96, None) == -1 and b'multiple of 64' in lib.sl_last_error_string()
    assert lib.sl_stem_bn_relu_pool_fwd_c(bf, d, d, d, d, None, 2, 32, 32, 2048, None) == -1
    assert lib.sl_stem_bn_relu_pool_fwd_c(bf, None, d, d, d, None, 2, 32, 32, 128, None) == -1
    assert lib.sl_stem_pool_relu_bwd_bnstat_c(bf, d, d, d, d, d, d, d, d, None, 2, 32, 32, 128, None) == -1                                 # no partial buffer
    assert lib.sl_stem_pool_relu_bwd_bnstat_c(f32, d, d, d, d, d, d, d, d, d, 2, 32, 32, 100, None) == -1
    assert lib.sl_stem_pool_relu_bwd_bnstat_c(5, d, d, d, d, d, d, d, d, d, 2, 32, 32, 128, None) == -1


def test_launch_plan_queries(lib):
    """Rows of the statistic partials from the launch plans: bench shape (B 16, 512 x 512) and a ragged one."""
    assert lib.sl_stem3_conv_stat_rows(16, 512, 512) == 16 * 16 * 16                  # one per 16 x 16 tile of the 256 x 256 output
    assert lib.sl_stem3_conv_stat_rows(3, 50, 78) == 3 * 2 * 3                        # 25 x 39 output: the tile grid rounds up
    assert lib.sl_stem3_conv_stat_rows(0, 64, 64) == 0
    assert lib.sl_stem3_conv_fwd_workspace(_lib.SL_BF16) == 8192 and lib.sl_stem3_conv_fwd_workspace(_lib.SL_F32) == 0
    assert lib.sl_stem3_conv_bwd_weight_workspace(16, 512, 512) == 512 * 64 * 27 * 4  # persistent blocks: at most 512 partials
    assert lib.sl_stem_pool_relu_bwd_bnstat_c_rows(16, 256, 256, 128) == 2048         # capped
    assert lib.sl_stem_pool_relu_bwd_bnstat_c_rows(3, 13, 22, 128) == (3 * 13 * 22 * 16 + 255) // 256
    assert lib.sl_stem_pool_relu_bwd_bnstat_c_rows(2, 24, 40, 64) == lib.sl_stem_pool_relu_bwd_bnstat_rows(2, 24, 40)
    assert lib.sl_stem_pool_relu_bwd_bnstat_c_rows(2, 24, 40, 96) == 0
    # the conv layers behind conv1 at 1 048 576 rows: which kernel, and the rows their statistic partials have
    bf = _lib.SL_BF16
    d2 = _lib.SlConvDesc(bf, 16, 256, 256, 64, 64, 3, 3, 1, 1, 1, 256, 256, 64)
    d3 = _lib.SlConvDesc(bf, 16, 256, 256, 64, 128, 3, 3, 1, 1, 1, 256, 256, 64)
    assert lib.sl_conv2d_tile_config_ex(C.byref(d2), 0, 1) == 7016016 and lib.sl_conv2d_stat_rows(C.byref(d2)) == 4096
    assert lib.sl_conv2d_tile_config_ex(C.byref(d3), 0, 1) == 4256128 and lib.sl_conv2d_stat_rows(C.byref(d3)) == 4096
    assert lib.sl_conv2d_wgrad_config(C.byref(d2)) == 1 and lib.sl_conv2d_wgrad_config(C.byref(d3)) == 3
    assert 0 < lib.sl_conv2d_bwd_weight_workspace(C.byref(d3)) < (1 << 30)


def test_restatement_reproduces_g20():
    g = golden('g20_deep_stem')
    ora = rv.DeepStemResNet((3, 4, 6, 3))
    ora.load_state_dict({k: fm.formula_tensor('g20/' + k, v) for k, v in ora.state_dict().items()})
    ora.train()
    img = fm.formula_image(2, 64, 64, 'g20/img')
    y = ora.stem(img)
    (y * fm.sym('g20/coef', tuple(y.shape), 1.0)).sum().backward()
    assert np.array_equal(y.detach().numpy(), g['y'])
    for n in ('conv1', 'conv2', 'conv3'):
        assert np.array_equal(getattr(ora, n).weight.grad.numpy(), g['d_%s_w' % n]), n
    for n in ('bn1', 'bn2', 'bn3'):
        bn = getattr(ora, n)
        assert np.array_equal(bn.weight.grad.numpy(), g['d_%s_gamma' % n]) and np.array_equal(bn.bias.grad.numpy(), g['d_%s_beta' % n]), n
        assert np.array_equal(bn.running_mean.numpy(), g['rm_' + n]) and np.array_equal(bn.running_var.numpy(), g['rv_' + n]), n
    ora.eval()
    with torch.no_grad():
        assert np.array_equal(ora.stem(img).numpy(), g['y_eval'])


@pytest.mark.slow
def test_restatement_reproduces_g21():
    g = golden('g21_full_r50v2')
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    ora = fm.load_formula_weights(rv.PopV2(n_base=7, criterion=po.OrthLossOracle(255))).train()
    img = fm.formula_image(2, 512, 512, 'g6/img')
    mask = fm.formula_mask(2, 512, 512, 8, 'g6/mask')
    crit, ora.criterion = ora.criterion, None
    logits = ora(img)
    ora.criterion = crit
    assert np.array_equal(logits.detach().numpy(), g['logits'])
    e = F.normalize(ora.base_emb.unsqueeze(0), p=2, dim=-1).squeeze(0)
    d = crit(logits, mask, proto_sim=e @ e.t())
    d['total_loss'].backward()
    assert float(d['total_loss']) == float(g['total']) and float(d['seg_loss']) == float(g['seg']) and float(d['orth_loss']) == float(g['orth'])
    bb = ora.backbone
    assert np.array_equal(bb.conv1.weight.grad.numpy(), g['d_conv1']) and np.array_equal(bb.conv3.weight.grad.numpy(), g['d_conv3'])
    assert np.array_equal(bb.layer1[0].downsample[0].weight.grad[:, :, 0, 0].numpy(), g['d_l1_ds'])
    assert np.array_equal(ora.base_emb.grad.numpy(), g['d_base_emb'])
