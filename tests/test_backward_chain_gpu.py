"""The master switch of the BatchNorm-backward fusions (functional._BN_FUSE, SEGLAND_BN_FUSE=0) at model level: with it and the two hooks derived from it off, no
data-gradient or pool-backward epilogue produces column sums and every ops.bn_bwd runs its own reduce pass; with them on, every fused route is taken; the two backward
chains give the same loss and the same parameter gradients up to the summation order of the column sums."""
import inspect

import pytest
import torch

from oracle import formula as fm

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# wrapper -> was the call served with column sums?
FUSED = {'conv2d_bwd_data_bnstat': lambda out: out is not None, 'conv2d_bwd_data_addend_bnstat': lambda out: out is not None,
         'conv2d_bwd_data_addend_bnstat2': lambda out: out is not None, 'conv2d_bwd_data_addend_half': lambda out: out[1] is not None,
         'stem_pool_relu_bwd_bnstat': lambda out: True}


def test_master_switch_of_the_bn_backward_fusions(hip):
    """R50 bf16, 4 tiles of 512 x 512: the smallest batch at which layer1 and layer2's first block have the 65 536 rows the pixel-stationary kernel takes, so the
    epilogue (bnstat), cross-block, dual and half-resolution routes all occur.
    Gates: those of test_round3_gpu.py's fused-against-unfused comparison (global relative L2 1e-2, worst tensor 6e-2; fused and unfused differ in the summation order of
    the column sums only, which the train-mode BatchNorm chain of an untrained network amplifies).  Measured at this shape, on the parent of the change that added
    this test and on the change itself alike: global 4.87e-3, worst tensor 2.33e-2 (backbone.layer1.0.bn1.bias); 36 of 46 ops.bn_bwd calls arrive with column sums (off: 0 of 58)."""
    from segland_amd import functional as sf, ops
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.networks.pspnet_pop import GFSS_Model
    img = fm.formula_image(4, 512, 512, 'chain/img').to(DEV)
    mask = fm.formula_mask(4, 512, 512, 8, 'chain/mask', block=32, ignore_rows=40).to(DEV)
    torch.manual_seed(3)
    m = GFSS_Model(n_base=7, criterion=OrthLoss(255), backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=torch.bfloat16).to(DEV).train()
    served, pre_partials = {}, []
    real = {name: getattr(ops, name) for name in list(FUSED) + ['bn_bwd']}
    bn_bwd_sig = inspect.signature(real['bn_bwd'])

    def counted(name):
        def f(*a, **k):
            out = real[name](*a, **k)
            served[name] += bool(FUSED[name](out))
            return out
        return f

    def bn_bwd(*a, **k):
        pre_partials.append(bn_bwd_sig.bind(*a, **k).arguments.get('pre_partial') is not None)
        return real['bn_bwd'](*a, **k)
    hooks = {name: getattr(sf, name) for name in ('_BN_FUSE', '_BN_DUAL', '_BN_CROSS')}
    runs = {}
    try:
        for name in FUSED:
            setattr(ops, name, counted(name))
        ops.bn_bwd = bn_bwd
        for flag in (False, True):
            sf._BN_FUSE = sf._BN_DUAL = sf._BN_CROSS = flag
            served.update({name: 0 for name in FUSED})
            del pre_partials[:]
            m.zero_grad(set_to_none=True)
            d = m(img, mask)
            d['total_loss'].backward()
            runs[flag] = ({k: p.grad.detach().float().clone() for k, p in m.named_parameters() if p.grad is not None}, dict(served), list(pre_partials),
                          float(d['total_loss'].detach()))
    finally:
        for name, fn in real.items():
            setattr(ops, name, fn)
        for name, v in hooks.items():
            setattr(sf, name, v)
    (g0, n0, pp0, l0), (g1, n1, pp1, l1) = runs[False], runs[True]
    num = sum(float(((g1[k] - v) ** 2).sum()) for k, v in g0.items())
    den = sum(float((v ** 2).sum()) for v in g0.values())
    worst = max((float((g1[k] - v).norm() / max(float(v.norm()), 1e-20)), k) for k, v in g0.items())
    print('switch off: served %s, bn_bwd calls %d (with column sums: %d); on: served %s, bn_bwd calls %d (with column sums: %d)' % (n0, len(pp0), sum(pp0), n1, len(pp1), sum(pp1)))
    print('loss %.6f / %.6f; gradients fused vs unfused: global rel. L2 %.2e, worst tensor %.2e (%s)' % (l1, l0, (num / den) ** 0.5, worst[0], worst[1]))
    assert all(v == 0 for v in n0.values()) and pp0 and not any(pp0), (n0, pp0)
    assert all(v >= 1 for v in n1.values()), n1
    # no column sums are lost on the way: each set an epilogue served reaches one ops.bn_bwd call, except the dual pair, which goes to ops.bn_bwd2
    assert sum(pp1) == sum(n1.values()) - n1['conv2d_bwd_data_addend_bnstat2'], (n1, sum(pp1))
    assert l0 == l1 and g0.keys() == g1.keys()
    assert (num / den) ** 0.5 <= 1e-2 and worst[0] <= 6e-2
