"""Wide POP head (more than 16 prototypes), CPU side: golden G23 (tests/golden/make_golden_v3.py: the reference at 20 base and 15 + 5 prototypes, 21 logit channels)
pins oracle/pop_oracle.py at that width -- forward values torch.equal, gradients to 1e-6, the gates make_golden.g2 applies before it stores anything -- the collapsed head
identity the HIP kernels rely on holds at K = 20, and the library names its limit (32 prototypes, 33 logit channels) when it refuses a wider call, before any launch."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import formula as fm
from oracle import pop_oracle as po


def build(n_base, is_ft=False, n_novel=0):
    m = po.PopOracle(n_base=n_base, criterion=po.OrthLossOracle(255), is_ft=is_ft, n_novel=n_novel, backbone='resnet50')
    return fm.load_formula_weights(m)


def equal(got, ref, what):
    ref = torch.from_numpy(ref)
    assert torch.equal(got.detach(), ref), '%s: max abs difference %g' % (what, float((got.detach() - ref).abs().max()))


def close6(got, ref, what):
    ref = torch.from_numpy(ref)
    assert torch.allclose(got.detach(), ref, rtol=1e-6, atol=1e-6), '%s: max abs difference %g' % (what, float((got.detach() - ref).abs().max()))


def test_g23_head_base_and_all():
    g = golden('g23_wide_head')
    m = build(20)
    feats = fm.sym('g23/feats', (2, 512, 8, 8), 1.0).requires_grad_(True)
    coef = fm.sym('g23/coef', (2, 21, 8, 8), 1.0)
    preds = po.head_base(m, feats)
    assert tuple(preds.shape) == (2, 21, 8, 8)
    (preds * coef).sum().backward()
    equal(preds, g['preds'], 'preds')
    close6(feats.grad, g['dfeats'], 'dfeats')
    close6(m.base_emb.grad, g['d_base_emb'], 'd_base_emb')
    close6(m.classifier[0].weight.grad[::8, ::8, 0, 0], g['d_cls0'], 'd_cls0')
    close6(m.classifier[2].weight.grad[::8, ::8, 0, 0], g['d_cls2'], 'd_cls2')
    close6(m.classifier[4].weight.grad[0, :, 0, 0], g['d_cls4'], 'd_cls4')
    m2 = build(15, True, 5).eval()
    pa = po.head_all(m2, feats.detach())[0]
    assert tuple(pa.shape) == (2, 21, 8, 8)
    equal(pa, golden('g23_wide_head_all')['preds'], 'preds_all')


def test_g23_loss():
    g = golden('g23_wide_head_loss')
    co = po.OrthLossOracle(255)
    preds = fm.sym('g23/preds', (2, 21, 8, 8), 2.0).requires_grad_(True)
    target = fm.formula_mask(2, 64, 64, 21, tag='g23/mask', block=8, ignore_rows=5)
    assert sorted(target.unique().tolist()) == list(range(21)) + [255]
    rect = fm.sym('g23/rect', (5, 20), 1.0)
    d = co(preds, target, is_ft=True, proto_sim=rect)
    d['total_loss'].backward()
    equal(d['total_loss'], g['total'], 'total'); equal(d['seg_loss'], g['seg'], 'seg'); equal(d['orth_loss'], g['orth'], 'orth')
    close6(preds.grad, g['dpreds'], 'dpreds')


def test_head_collapse_identity_k20():
    """pred = a_k max(p, 0) + b_k max(-p, 0) with a_k = MLP(s_k), b_k = MLP(-s_k) (test_oracle_golden.test_head_collapse_identity) at 20 prototypes."""
    m = build(20)
    feats = fm.sym('g23/feats', (2, 512, 8, 8), 1.0)
    preds = po.head_base(m, feats)
    s = F.normalize(m.base_emb.detach(), dim=-1)
    p = torch.einsum('kc,bcn->bkn', s, feats.flatten(2))
    ab = po.classifier_forward(m.classifier, torch.cat([s, -s], 0).view(40, 512, 1, 1)).view(2, 20)
    fg = ab[0].view(1, 20, 1) * p.clamp(min=0) + ab[1].view(1, 20, 1) * (-p).clamp(min=0)
    torch.testing.assert_close(fg.view(2, 20, 8, 8), preds[:, 1:].detach(), rtol=1e-4, atol=1e-5)


@pytest.fixture(scope='module')
def lib():
    import os
    from segland_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_limits_are_named_before_any_launch(lib):
    """33 prototypes / 34 logit channels are refused during argument validation (no device needed) and the message carries the limit."""
    d = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string().decode()
    for dtype in (0, 1):
        assert lib.sl_pop_decompose_fwd(dtype, d, d, 33, d, d, 48, 512, None) == -1 and '33 prototypes' in err() and 'at most 32' in err()
        assert lib.sl_pop_decompose_bwd(dtype, d, d, d, d, d, 33, d, d, 48, 512, None) == -1 and 'at most 32' in err()
    assert lib.sl_pop_combine_fwd(d, d, d, d, 33, d, 2, 24, None) == -1 and 'at most 32' in err()
    assert lib.sl_pop_combine_bwd(d, d, d, d, 33, d, d, d, 2, 24, None) == -1 and 'at most 32' in err()
    assert lib.sl_upsample_ce_fwd(d, d, 2, 34, 8, 8, 64, 64, 255, d, None) == -1 and '34 logit channels' in err() and 'at most 33' in err()
    assert lib.sl_upsample_ce_bwd(d, d, d, d, 2, 34, 8, 8, 64, 64, 255, d, None) == -1 and 'at most 33' in err()
    assert lib.sl_pseudo_label(d, 34, 8, 8, d, 2, 64, 64, 15, None) == -1 and 'at most 33' in err()
    assert lib.sl_upsample_argmax(d, 2, 34, 8, 8, 64, 64, d, None) == -1 and 'at most 33' in err()
    assert lib.sl_upsample_logits(d, 2, 34, 8, 8, 64, 64, d, None) == -1 and 'at most 33' in err()
