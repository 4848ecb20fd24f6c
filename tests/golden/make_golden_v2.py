#!/usr/bin/env python3
"""Golden records of the deep-stem backbones (G20, G21, G22), generated from the REFERENCE on the build machine only.

Reuses the reference import, save() and same() of make_golden.py.  The reference's ResNetv2 and GFSS_Model(backbone='resnet50v2') and the CPU restatement
(tests/resnetv2_cpu.py) get the same formula weights; outputs and gradients must be torch.equal before anything is written.  Only arrays and the list of
state_dict key names are stored.

    python tests/golden/make_golden_v2.py [g20 g21 g22]
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                      # noqa: E402  (imports the reference with its stubs)
from make_golden import fm, po, same, save    # noqa: E402
import resnetv2_cpu as rv                     # noqa: E402
from networks.backbones.resnet import ResNetv2 as RefResNetv2   # noqa: E402


def g20():
    ref = RefResNetv2(mg.RefBottleneck, [3, 4, 6, 3])
    ora = rv.DeepStemResNet((3, 4, 6, 3))
    assert list(ref.state_dict().keys()) == list(ora.state_dict().keys())
    sd = {k: fm.formula_tensor('g20/' + k, v) for k, v in ref.state_dict().items()}
    ref.load_state_dict(sd); ora.load_state_dict(sd)
    img = fm.formula_image(2, 64, 64, 'g20/img')
    ref.train(); ora.train()
    y = ref.forward_base_in(img)
    coef = fm.sym('g20/coef', tuple(y.shape), 1.0)
    (y * coef).sum().backward()
    yo = ora.stem(img)
    (yo * coef).sum().backward()
    same(y, yo, 'g20 y')
    out = dict(y=y)
    for n in ('conv1', 'conv2', 'conv3'):
        same(getattr(ref, n).weight.grad, getattr(ora, n).weight.grad, 'g20 d' + n)
        out['d_%s_w' % n] = getattr(ref, n).weight.grad
    for n in ('bn1', 'bn2', 'bn3'):
        r, o = getattr(ref, n), getattr(ora, n)
        same(r.weight.grad, o.weight.grad, 'g20 dgamma ' + n); same(r.bias.grad, o.bias.grad, 'g20 dbeta ' + n)
        same(r.running_mean, o.running_mean, 'g20 rm ' + n); same(r.running_var, o.running_var, 'g20 rv ' + n)
        out.update({'d_%s_gamma' % n: r.weight.grad, 'd_%s_beta' % n: r.bias.grad, 'rm_' + n: r.running_mean, 'rv_' + n: r.running_var})
    ref.eval(); ora.eval()
    ye = ref.forward_base_in(img)
    same(ye, ora.stem(img), 'g20 y_eval')
    save('g20_deep_stem', y_eval=ye, **out)


def build_pair_v2(is_ft=False, n_novel=0):
    ref = mg.ref_pop.GFSS_Model(n_base=7, criterion=mg.RefOrthLoss(ignore_index=255), is_ft=is_ft, n_novel=n_novel, backbone='resnet50v2',
                                pretrained_model=None, dilated=True, os=8)
    ora = rv.PopV2(n_base=7, criterion=po.OrthLossOracle(ignore_index=255), is_ft=is_ft, n_novel=n_novel, backbone='resnet50v2')
    assert list(ref.state_dict().keys()) == list(ora.state_dict().keys()), 'state_dict keys differ'
    sd = fm.formula_state_dict(ref)
    ref.load_state_dict(sd, strict=True); ora.load_state_dict(sd, strict=True)
    return ref, ora


def g21():
    ref, ora = build_pair_v2()
    img = fm.formula_image(2, 512, 512, 'g6/img')
    mask = fm.formula_mask(2, 512, 512, 8, 'g6/mask')
    ref.train(); ora.train()
    crit = ref.criterion
    ref.criterion = None
    logits = ref(img)
    ref.criterion = crit
    sim_e = F.normalize(ref.base_emb.unsqueeze(0), p=2, dim=-1).squeeze(0)
    loss = crit(logits, mask, proto_sim=sim_e @ sim_e.t())
    loss['total_loss'].backward()
    gnorm = torch.nn.utils.clip_grad_norm_(ref.parameters(), 1e30)
    lo = ora(img, mask)
    lo['total_loss'].backward()
    gnorm_o = torch.nn.utils.clip_grad_norm_(ora.parameters(), 1e30)
    for k in loss:
        same(loss[k], lo[k], 'g21 ' + k)
    same(gnorm, gnorm_o, 'g21 gnorm')
    rb, ob = ref.backbone, ora.backbone
    stem_w = {'d_conv1': (rb.conv1, ob.conv1), 'd_conv2': (rb.conv2, ob.conv2), 'd_conv3': (rb.conv3, ob.conv3),
              'd_l1_conv1': (rb.layer1[0].conv1, ob.layer1[0].conv1), 'd_l1_ds': (rb.layer1[0].downsample[0], ob.layer1[0].downsample[0])}
    for k, (r, o) in stem_w.items():
        same(r.weight.grad, o.weight.grad, 'g21 ' + k)
    same(ref.base_emb.grad, ora.base_emb.grad, 'g21 d_base_emb')
    up = F.interpolate(logits, size=(512, 512), mode='bilinear', align_corners=True)
    amax = up.argmax(1).to(torch.uint8)
    ref.eval()
    logits_eval = ref(img)
    gn = {k: p.grad.norm() for k, p in ref.named_parameters()}
    keys = sorted(gn)
    save('g21_full_r50v2', logits=logits, argmax=amax, total=loss['total_loss'], seg=loss['seg_loss'], orth=loss['orth_loss'],
         gnorm=gnorm, d_base_emb=ref.base_emb.grad, d_cls4=ref.classifier[4].weight.grad[0, :, 0, 0], d_dec_bias=ref.decoder.bottleneck[3].bias.grad,
         rm_bn1=rb.bn1.running_mean, rv_bn1=rb.bn1.running_var, rm_bn3=rb.bn3.running_mean, rv_bn3=rb.bn3.running_var, rm_l4=rb.layer4[2].bn3.running_mean,
         grad_norm_keys=np.array(keys), grad_norms=torch.stack([gn[k] for k in keys]),
         state_dict_keys=np.array(list(ref.state_dict().keys())), state_dict_shapes=np.array(['x'.join(map(str, v.shape)) for v in ref.state_dict().values()]),
         **{k: r.weight.grad[:, :, 0, 0] if r.weight.shape[-1] == 1 else r.weight.grad for k, (r, _) in stem_w.items()})
    # save() moves the largest quarter of the arrays into ONE .part2 file; with both logit tensors in the record that part is 1 065 595 bytes, over the limit of a
    # committed file, so the eval logits are a part of their own (conftest.golden merges every <name>.part*.npz)
    np.savez_compressed(os.path.join(HERE, 'g21_full_r50v2.part3.npz'), logits_eval=logits_eval.detach().numpy())


def g22():
    ref, ora = build_pair_v2(is_ft=True, n_novel=4)
    ref.init_cls_n(); po.init_cls_n(ora)
    with torch.no_grad():
        for (k, p), (_, q) in zip(ref.classifier_n.named_parameters(), ora.classifier_n.named_parameters()):
            p.add_(fm.sym('g7/cn/' + k, tuple(p.shape), 0.01)); q.copy_(p)
    img = fm.formula_image(1, 512, 512, 'g7/img')
    img_b = fm.formula_image(1, 512, 512, 'g7/img_b')
    mask = fm.formula_mask(1, 512, 512, 4, 'g7/mask', ignore_rows=0, lo=8)
    mask[mask == 8] = 255
    mask_b = fm.formula_mask(1, 512, 512, 8, 'g7/mask_b', ignore_rows=0)
    mb_r, mb_o = mask_b.clone(), mask_b.clone()
    ref.train_mode(); po.train_mode(ora)
    d = ref(img, mask, img_b, mb_r)
    d['total_loss'].backward()
    do = ora(img, mask, img_b, mb_o)
    do['total_loss'].backward()
    for k in d:
        same(d[k], do[k], 'g22 ' + k)
    assert torch.equal(mb_r, mb_o), 'g22 pseudo labels differ'
    same(ref.novel_emb.grad, ora.novel_emb.grad, 'g22 dnovel', 1e-6)      # as G7: the oracle's head sums this gradient in another order (last-bit differences); losses and labels are equal
    crit = ref.criterion
    ref.criterion = None
    preds = ref(img, mask, img_b, mask_b.clone())
    ref.criterion = crit
    ref.eval()
    pall = ref(img)
    save('g22_ft_v2', preds=preds, preds_all=pall, d_clsn0=ref.classifier_n[0].weight.grad[::8, ::8, 0, 0], mask_b_new=mb_r.to(torch.uint8), total=d['total_loss'], seg=d['seg_loss'], orth=d['orth_loss'],
         d_novel_emb=ref.novel_emb.grad, d_clsn4=ref.classifier_n[4].weight.grad[0, :, 0, 0])


ALL = dict(g20=g20, g21=g21, g22=g22)

if __name__ == '__main__':
    for w in sys.argv[1:] or list(ALL):
        print('==', w)
        ALL[w]()
