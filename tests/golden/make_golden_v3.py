#!/usr/bin/env python3
"""Golden records of the wide POP head (G23: more than 16 prototypes), generated from the REFERENCE on the build machine only.

Reuses the reference import, save() and same() of make_golden.py.  The reference's GFSS_Model and po.PopOracle get the same formula weights; outputs must be
torch.equal (gradients 1e-6, as in g2()) before anything is written.  Only arrays are stored.

    python tests/golden/make_golden_v3.py [g23]
"""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                      # noqa: E402  (imports the reference with its stubs)
from make_golden import fm, po, same, save    # noqa: E402


def build_pair_wide(n_base, is_ft=False, n_novel=0):
    ref = mg.ref_pop.GFSS_Model(n_base=n_base, criterion=mg.RefOrthLoss(ignore_index=255), is_ft=is_ft, n_novel=n_novel, backbone='resnet50',
                                pretrained_model=None, dilated=True, os=8)
    ora = po.PopOracle(n_base=n_base, criterion=po.OrthLossOracle(ignore_index=255), is_ft=is_ft, n_novel=n_novel, backbone='resnet50')
    assert list(ref.state_dict().keys()) == list(ora.state_dict().keys()), 'state_dict keys differ'
    sd = fm.formula_state_dict(ref)
    ref.load_state_dict(sd, strict=True)
    ora.load_state_dict(sd, strict=True)
    return ref, ora


def g23():
    # base head, 20 prototypes (21 logit channels)
    ref, ora = build_pair_wide(20)
    mg._head_only(ref)
    feats = fm.sym('g23/feats', (2, 512, 8, 8), 1.0).requires_grad_(True)
    coef = fm.sym('g23/coef', (2, 21, 8, 8), 1.0)
    ref.criterion = None
    preds = ref(feats)
    (preds * coef).sum().backward()
    feats_o = feats.detach().clone().requires_grad_(True)
    preds_o = po.head_base(ora, feats_o)
    (preds_o * coef).sum().backward()
    same(preds, preds_o, 'g23 preds')
    same(feats.grad, feats_o.grad, 'g23 dfeats', 1e-6)
    same(ref.base_emb.grad, ora.base_emb.grad, 'g23 demb', 1e-6)
    save('g23_wide_head', preds=preds, dfeats=feats.grad, d_base_emb=ref.base_emb.grad,
         d_cls0=ref.classifier[0].weight.grad[::8, ::8, 0, 0], d_cls2=ref.classifier[2].weight.grad[::8, ::8, 0, 0],
         d_cls4=ref.classifier[4].weight.grad[0, :, 0, 0])
    # ft head (forward_all), 15 base + 5 novel prototypes, on the same feats
    ref, ora = build_pair_wide(15, is_ft=True, n_novel=5)
    mg._head_only(ref)
    ref.eval(); ora.eval()
    pa = ref(feats.detach())
    pa_o, _ = po.head_all(ora, feats.detach())
    same(pa, pa_o, 'g23 preds_all')
    save('g23_wide_head_all', preds=pa)
    # loss: 21 classes, rectangular [novel, novel + base] prototype similarity of the fine-tune stage
    cr, co = mg.RefOrthLoss(ignore_index=255), po.OrthLossOracle(ignore_index=255)
    lp = fm.sym('g23/preds', (2, 21, 8, 8), 2.0).requires_grad_(True)
    target = fm.formula_mask(2, 64, 64, 21, tag='g23/mask', block=8, ignore_rows=5)
    rect = fm.sym('g23/rect', (5, 20), 1.0)
    d = cr(lp, target, is_ft=True, proto_sim=rect)
    d['total_loss'].backward()
    lp_o = lp.detach().clone().requires_grad_(True)
    d_o = co(lp_o, target, is_ft=True, proto_sim=rect)
    d_o['total_loss'].backward()
    for k in d:
        same(d[k], d_o[k], 'g23 ' + k)
    same(lp.grad, lp_o.grad, 'g23 dpreds')
    save('g23_wide_head_loss', total=d['total_loss'], seg=d['seg_loss'], orth=d['orth_loss'], dpreds=lp.grad)


ALL = dict(g23=g23)

if __name__ == '__main__':
    for w in sys.argv[1:] or list(ALL):
        print('==', w)
        ALL[w]()
