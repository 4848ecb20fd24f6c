"""Wide POP head on the GPU: 17..32 prototypes (18..33 logit channels) through every kernel of the head -> loss -> label path, at the smallest shapes at which those
kernels can go wrong, and through the models (PSPNet-POP base and fine-tune mode, Swin-POP) against the CPU oracle evaluated on this machine.  Every kernel-level case
was refused with `bad args` before the wide kernels existed.  References are CPU fp32 torch (oracle/pop_oracle.py); the bounds are those of the narrow kernels' tests
(test_g1_decompose_gpu, test_g2_head, test_loss_vs_oracle_512, test_loss_backward_tiled_equals_gather, test_model_gpu G6 / G7, test_swin_gpu G16)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import formula as fm
from oracle import pop_oracle as po

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KTS = (17, 20, 31, 32)          # one past a chunk of 16, the PASCAL-5i count, odd, full


def protos(Kt, C):
    return F.normalize(fm.sym('wide/bb%d' % Kt, (1, Kt, C), 1.0), p=2, dim=-1)[0].contiguous()


def rows(x):                    # [B, C, N] -> [B*N, C]
    return x.permute(0, 2, 1).reshape(-1, x.shape[1]).contiguous()


def check(got, ref, tol, what):
    """forward quantities: max abs error relative to the tensor scale (test_model_gpu.check)"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    e = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)
    print('%s: max error %.3g of scale' % (what, e))
    assert e <= tol, '%s: max error %.3g of scale (tolerance %.1g)' % (what, e, tol)


def check_grad(got, ref, tol, what):
    """gradients: relative L2 error <= tol and at most 0.05 % of the elements further than 10 tol scale away (test_model_gpu.check_grad)"""
    got, ref = got.detach().float().cpu().numpy(), ref.detach().float().cpu().numpy()
    l2 = float(np.linalg.norm((got - ref).ravel()) / max(np.linalg.norm(ref.ravel()), 1e-20))
    out = float((np.abs(got - ref) > 10 * tol * np.abs(ref).max()).mean())
    print('%s: relative L2 %.3g, outliers %.4f%%' % (what, l2, 100 * out))
    assert l2 <= tol, '%s: relative L2 error %.3g (tolerance %.1g)' % (what, l2, tol)
    assert out <= 5e-4, '%s: %.4f%% outliers' % (what, 100 * out)


# --------------------------------------------------------------------------------------------- 1. decompose forward
@pytest.mark.parametrize('dtype,C', [(torch.float32, 512), (torch.bfloat16, 512), (torch.float32, 128), (torch.bfloat16, 128), (torch.bfloat16, 256)])
def test_decompose_fwd_wide(hip, dtype, C):
    """proj and the background residual against po.orthogonal_decompose (CPU fp32): 2e-6 of the largest magnitude for fp32 storage (test_g1_decompose_gpu; the fp32 oracle
    is itself 2-5e-7 from a float64 evaluation on these inputs), 2e-2 for bf16 storage.  R = 50 leaves a ragged last row group at 4 and 2 rows per wavefront."""
    from segland_amd import ops
    tol = 2e-6 if dtype == torch.float32 else 2e-2
    for N in (24, 25):
        feats = fm.sym('wide/feats', (2, C, N), 1.0)
        f2d = rows(feats).to(DEV).to(dtype)
        for Kt in KTS:
            S = protos(Kt, C)
            _, bg_ref = po.orthogonal_decompose(feats, S.unsqueeze(0))
            proj_ref = torch.matmul(S.unsqueeze(0), feats)
            bg = torch.empty_like(f2d)
            proj = ops.pop_decompose_into(f2d, S.to(DEV), bg)
            got_proj = proj.view(2, N, Kt).permute(0, 2, 1).cpu()
            got_bg = bg.float().view(2, N, C).permute(0, 2, 1).cpu()
            ep = float((got_proj - proj_ref).abs().max() / proj_ref.abs().max())
            eb = float((got_bg - bg_ref[:, 0]).abs().max() / bg_ref.abs().max())
            print('decompose fwd %s C %d R %d Kt %d: proj %.3g bg %.3g of the maximum' % (dtype, C, 2 * N, Kt, ep, eb))
            assert ep <= tol and eb <= tol, (Kt, N, ep, eb)
            bg2 = torch.empty_like(f2d)
            assert torch.equal(ops.pop_decompose_into(f2d, S.to(DEV), bg2), proj) and torch.equal(bg2, bg), 'run-to-run'


# --------------------------------------------------------------------------------------------- 2. decompose backward, combine forward / backward
@pytest.mark.parametrize('C', [512, 128])
@pytest.mark.parametrize('Kt', KTS)
def test_decompose_bwd_and_combine_wide(hip, Kt, C):
    """fp32, R = 48: autograd through po.orthogonal_decompose and the combine formula in torch.  The oracle normalises its bases, so its prototype gradient is the
    tangential part (I - s s^T) dS of the kernel's dS (the radial part never leaves ProtoFn either); tolerances of test_g2_head (1e-3 of scale forward, 1e-2 relative L2
    on gradients).  Two runs of each wide kernel are bit-equal."""
    from segland_amd import ops
    B, N = 2, 24
    feats = fm.sym('wide/feats', (B, C, N), 1.0)
    S = protos(Kt, C)
    cg = fm.sym('wide/cg', (B, C, N), 1.0)                   # d loss / d bg
    cp = fm.sym('wide/cp%d' % Kt, (B, 1 + Kt, N), 1.0)       # d loss / d preds
    q = feats.clone().requires_grad_(True)
    E = S.clone().unsqueeze(0).requires_grad_(True)
    zbg = fm.sym('wide/zbg', (B, N), 1.0).requires_grad_(True)
    a = fm.sym('wide/a%d' % Kt, (Kt,), 1.0).requires_grad_(True)
    b = fm.sym('wide/b%d' % Kt, (Kt,), 1.0).requires_grad_(True)
    _, bg = po.orthogonal_decompose(q, E)
    proj = torch.matmul(F.normalize(E, p=2, dim=-1), q)      # the oracle's own expression for the projections
    proj.retain_grad()
    preds = torch.cat([zbg.unsqueeze(1), a.view(1, -1, 1) * proj.clamp(min=0) + b.view(1, -1, 1) * (-proj).clamp(min=0)], 1)
    ((bg[:, 0] * cg).sum() + (preds * cp).sum()).backward()

    f2d, Sg = rows(feats).to(DEV), S.to(DEV)
    bgg = torch.empty_like(f2d)
    pg = ops.pop_decompose_into(f2d, Sg, bgg)
    ag, bg_, zg = a.detach().to(DEV), b.detach().to(DEV), zbg.detach().reshape(-1).to(DEV)
    pr = ops.pop_combine_fwd(pg, zg, ag, bg_, B, N)
    check(pr, preds, 1e-3, 'combine fwd preds (Kt %d, C %d)' % (Kt, C))
    dz, dproj, da, db = ops.pop_combine_bwd(cp.to(DEV), pg, ag, bg_, B, N)
    check_grad(dz.view(B, N), zbg.grad, 1e-2, 'dz_bg')
    check_grad(dproj.view(B, N, Kt).permute(0, 2, 1), proj.grad, 1e-2, 'dproj')
    check_grad(da, a.grad, 1e-2, 'da'); check_grad(db, b.grad, 1e-2, 'db')
    dq, dS = ops.pop_decompose_bwd(rows(cg).to(DEV), f2d, Sg, pg, dproj)
    check_grad(dq.view(B, N, C).permute(0, 2, 1), q.grad, 1e-2, 'dq')
    tang = dS - Sg * (Sg * dS).sum(-1, keepdim=True)
    check_grad(tang, E.grad[0], 1e-2, 'dS (tangential part)')
    # full dS against the closed form on the CPU: dS_k = sum_r t_k q_r - p_k dg_r with t_k = dproj_k - dg_r . s_k
    q2, g2, p2, dp2 = rows(feats), rows(cg), pg.cpu(), dproj.cpu()
    t = dp2 - g2 @ S.t()
    check_grad(dS, t.t() @ q2 - p2.t() @ g2, 1e-2, 'dS (closed form)')
    dz2, dproj2, da2, db2 = ops.pop_combine_bwd(cp.to(DEV), pg, ag, bg_, B, N)
    dq2, dS2 = ops.pop_decompose_bwd(rows(cg).to(DEV), f2d, Sg, pg, dproj)
    assert torch.equal(pr, ops.pop_combine_fwd(pg, zg, ag, bg_, B, N))
    assert torch.equal(dz, dz2) and torch.equal(dproj, dproj2) and torch.equal(da, da2) and torch.equal(db, db2), 'combine bwd run-to-run'
    assert torch.equal(dq, dq2) and torch.equal(dS, dS2), 'decompose bwd run-to-run'


# --------------------------------------------------------------------------------------------- 3. cross-entropy
CE_CASES = [(17, (5, 6), (64, 64)), (21, (9, 7), (40, 33)), (33, (8, 8), (64, 64)), (33, (8, 8), (8, 8))]


@functools.lru_cache(maxsize=None)
def ce_reference(K, hw, HW):
    preds = fm.sym('wide/p%d' % K, (2, K) + hw, 3.0)
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='wide/m%d' % K, block=8, ignore_rows=5)
    pr = preds.clone().requires_grad_(True)
    ref = F.cross_entropy(F.interpolate(pr, size=HW, mode='bilinear', align_corners=True), target, ignore_index=255)
    (ref * 0.7).backward()
    return preds, target, float(ref.detach()), pr.grad.numpy()


@pytest.mark.parametrize('route', ['tiled', 'gather'])
@pytest.mark.parametrize('K,hw,HW', CE_CASES)
def test_upsample_ce_wide(hip, K, hw, HW, route):
    """Loss rtol 2e-5 (test_loss_vs_oracle_512), gradient rtol 1e-3 / atol 2e-8 (test_loss_backward_tiled_equals_gather) against torch fp32 (itself <= 3e-8 relative /
    5.6e-9 absolute from float64 on these inputs), the valid-pixel count exact; the channel-sliced tiled backward and, with the hook sl_debug_ce_tiled(0), the gather
    backward."""
    from segland_amd import ops
    preds, target, ref, dref = ce_reference(K, hw, HW)
    assert (K, hw, HW) == (33, (8, 8), (8, 8)) or len(target.unique()) == K + 1      # every class occurs (an 8 x 8 label map has one block)
    pg, tg = preds.to(DEV), target.to(DEV)
    out = ops.upsample_ce_fwd(pg, tg, 255)
    print('K %d %s -> %s: loss %.8g (torch %.8g), count %d' % (K, hw, HW, out[0].item(), ref, int(out[1].item())))
    np.testing.assert_allclose(out[0].item(), ref, rtol=2e-5)
    assert out[1].item() == float((target != 255).sum())
    if route == 'gather':
        hip.sl_debug_ce_tiled(0)
    gs = torch.full((1,), 0.7, device=DEV)
    dl = ops.upsample_ce_bwd(pg, tg, out, gs, 255)
    dl2 = ops.upsample_ce_bwd(pg, tg, out, gs, 255)
    print('   %s backward: max abs error %.3g (max |grad| %.3g)' % (route, float(np.abs(dl.cpu().numpy() - dref).max()), float(np.abs(dref).max())))
    assert torch.isfinite(dl).all() and torch.equal(dl, dl2)
    np.testing.assert_allclose(dl.cpu().numpy(), dref, rtol=1e-3, atol=2e-8)


def test_upsample_ce_g23(hip):
    """the 21-class loss record of golden G23 (generated from the reference)"""
    from segland_amd import ops
    g = golden('g23_wide_head_loss')
    preds = fm.sym('g23/preds', (2, 21, 8, 8), 2.0).to(DEV)
    target = fm.formula_mask(2, 64, 64, 21, tag='g23/mask', block=8, ignore_rows=5)
    out = ops.upsample_ce_fwd(preds, target.to(DEV), 255)
    np.testing.assert_allclose(out[0].item(), g['seg'], rtol=2e-5)
    assert out[1].item() == float((target != 255).sum())
    one = torch.ones(1, device=DEV)
    for tiled in (1, 0):
        hip.sl_debug_ce_tiled(tiled)
        dl = ops.upsample_ce_bwd(preds, target.to(DEV), out, one, 255)
        np.testing.assert_allclose(dl.cpu().numpy(), g['dpreds'], rtol=1e-3, atol=2e-8)


# --------------------------------------------------------------------------------------------- 4. labels, bit-exact
@pytest.mark.parametrize('K', [17, 21, 33])
def test_labels_wide_bitexact(hip, K):
    """upsample_argmax and pseudo_label_ against F.interpolate(...).argmax / po.pseudo_label, every pixel: the smallest top-2 margin of these inputs is 3.6e-4, 1.4e-4 and
    3.1e-5 (K = 17, 21, 33), far from a tie.  upsample_logits at K = 21 against F.interpolate (2e-6 of the largest magnitude)."""
    from segland_amd import ops
    HW = (40, 33)
    logits = fm.sym('wide/l%d' % K, (2, K, 9, 7), 2.0)
    up = F.interpolate(logits, size=HW, mode='bilinear', align_corners=True)
    t2 = up.topk(2, dim=1).values
    print('K %d: smallest top-2 margin %.3g' % (K, float((t2[:, 0] - t2[:, 1]).min())))
    am = ops.upsample_argmax(logits.to(DEV), HW).cpu()
    assert int((am.long() != up.argmax(1)).sum()) == 0
    mask = fm.formula_mask(2, HW[0], HW[1], 16, tag='wide/lm%d' % K, block=8, ignore_rows=0)       # 0..15: background + 15 base classes
    ref = mask.clone()
    for i in range(2):
        po.pseudo_label(logits[i], ref[i], 15)
    mg = mask.clone().to(DEV)
    ops.pseudo_label_(logits.to(DEV), mg, 15)
    assert int((mask == 0).sum()) > 0 and int((mg.cpu() != ref).sum()) == 0
    if K == 21:
        # 2e-6 of the largest magnitude, the form test_round2_gpu applies to this kernel.  An element-wise relative bound without an absolute floor cannot hold for any
        # fp32 evaluation: an interpolated value is a four-term sum of products of size <= max |logit| and may cancel to ~0 (measured: 2.0e-7 absolute = 1e-7 of the
        # maximum on 0.8 % of the elements, which is 4.9e-4 of such an element's own size)
        err = float((ops.upsample_logits(logits.to(DEV), HW).cpu() - up).abs().max())
        print('upsample_logits K 21: max abs error %.3g = %.3g of the maximum' % (err, err / float(up.abs().max())))
        assert err <= 2e-6 * float(up.abs().max())


# --------------------------------------------------------------------------------------------- 5. limits
def test_limits_and_narrow_route(hip):
    from segland_amd import ops
    f2d = rows(fm.sym('wide/feats', (2, 512, 24), 1.0)).to(DEV)
    with pytest.raises(RuntimeError, match='at most 32'):
        ops.pop_decompose_into(f2d, protos(33, 512).to(DEV), torch.empty_like(f2d))
    with pytest.raises(RuntimeError, match='at most 32'):
        ops.pop_combine_fwd(torch.zeros(48, 33, device=DEV), torch.zeros(48, device=DEV), torch.zeros(33, device=DEV), torch.zeros(33, device=DEV), 2, 24)
    lg = fm.sym('wide/p34', (2, 34, 8, 8), 3.0).to(DEV)
    tg = fm.formula_mask(2, 64, 64, 34, tag='wide/m34', block=8, ignore_rows=5).to(DEV)
    with pytest.raises(RuntimeError, match='at most 33'):
        ops.upsample_ce_fwd(lg, tg, 255)
    with pytest.raises(RuntimeError, match='at most 33'):
        ops.upsample_argmax(lg, (64, 64))
    # 16 prototypes / 16 channels: the kernels of the narrow route, run to run
    S = protos(16, 512).to(DEV)
    bg1, bg2 = torch.empty_like(f2d), torch.empty_like(f2d)
    assert torch.equal(ops.pop_decompose_into(f2d, S, bg1), ops.pop_decompose_into(f2d, S, bg2)) and torch.equal(bg1, bg2)
    l16, t16 = lg[:, :16].contiguous(), fm.formula_mask(2, 64, 64, 16, tag='wide/m16', block=8, ignore_rows=5).to(DEV)
    o1, o2 = ops.upsample_ce_fwd(l16, t16, 255), ops.upsample_ce_fwd(l16, t16, 255)
    one = torch.ones(1, device=DEV)
    assert torch.equal(o1, o2) and torch.equal(ops.upsample_ce_bwd(l16, t16, o1, one, 255), ops.upsample_ce_bwd(l16, t16, o1, one, 255))
    assert torch.equal(ops.upsample_argmax(l16, (64, 64)), ops.upsample_argmax(l16, (64, 64)))


# --------------------------------------------------------------------------------------------- models
def _pair(n_base, is_ft=False, n_novel=0):
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.networks.pspnet_pop import GFSS_Model
    kw = dict(n_base=n_base, is_ft=is_ft, n_novel=n_novel, backbone='resnet50')
    m = fm.load_formula_weights(GFSS_Model(criterion=OrthLoss(255), pretrained_model=None, dilated=True, os=8, compute_dtype=torch.float32, **kw))
    o = fm.load_formula_weights(po.PopOracle(criterion=po.OrthLossOracle(255), **kw))
    return m, o


def test_base_model_20_classes_vs_same_box_oracle(hip):
    """GFSS_Model(n_base=20) in train mode, fp32, B = 2, 64 x 64: logits to 1e-3 of scale, the three losses rtol 1e-4, base_emb.grad and classifier.4.weight.grad
    to the G6 tolerances of test_model_gpu.py (relative L2 1e-2)."""
    m, o = _pair(20)
    m = m.to(DEV).train(); o.train()
    img = fm.formula_image(2, 64, 64, 'wide/img')
    mask = fm.formula_mask(2, 64, 64, 21, 'wide/mask', block=8, ignore_rows=4)
    d = m(img.to(DEV), mask.to(DEV))
    d['total_loss'].backward()
    do = o(img, mask)
    do['total_loss'].backward()
    for k in do:
        print('%s: %.8g (oracle %.8g)' % (k, float(d[k].detach()), float(do[k].detach())))
        np.testing.assert_allclose(float(d[k].detach()), float(do[k].detach()), rtol=1e-4)
    check_grad(m.base_emb.grad, o.base_emb.grad, 1e-2, 'd_base_emb')
    check_grad(m.classifier[4].weight.grad[0, :, 0, 0], o.classifier[4].weight.grad[0, :, 0, 0], 1e-2, 'd_cls4')
    m.criterion = o.criterion = None
    with torch.no_grad():
        lg, lo = m(img.to(DEV)), o(img)
    assert tuple(lg.shape) == (2, 21, 8, 8)
    check(lg, lo, 1e-3, 'logits (train-mode BN)')


def test_ft_model_15_plus_5_vs_same_box_oracle(hip):
    """n_base=15, n_novel=5 in fine-tune mode, one novel and one base tile of 64 x 64: pseudo-labels equal the oracle's outside a 1e-5-of-scale top-2 margin (fewer than
    0.1 % of the pixels inside it), loss dict, novel_emb.grad (G7 tolerances), the eval-mode forward_all logits, and the evaluation path's confusion counts at 21 classes."""
    from segland_amd.eval_base import confusion_of_batch
    m, o = _pair(15, True, 5)
    m.init_cls_n(); po.init_cls_n(o)
    with torch.no_grad():
        for (k, p), (_, q) in zip(m.classifier_n.named_parameters(), o.classifier_n.named_parameters()):
            dlt = fm.sym('wide/cn/' + k, tuple(p.shape), 0.01)
            p.add_(dlt); q.add_(dlt)
    m = m.to(DEV)
    img, img_b = fm.formula_image(1, 64, 64, 'wide/ftimg'), fm.formula_image(1, 64, 64, 'wide/ftimg_b')
    mask = fm.formula_mask(1, 64, 64, 6, 'wide/ftmask', block=8, ignore_rows=0, lo=15); mask[mask == 15] = 255      # novel ids 16..20
    mask_b = fm.formula_mask(1, 64, 64, 16, 'wide/ftmask_b', block=8, ignore_rows=0)                                # background + 15 base classes
    mb_gpu, mb_cpu = mask_b.clone().to(DEV), mask_b.clone()
    m.train_mode(); po.train_mode(o)
    d = m(img.to(DEV), mask.to(DEV), img_b.to(DEV), mb_gpu)
    d['total_loss'].backward()
    do = o(img, mask, img_b, mb_cpu)
    do['total_loss'].backward()
    crit = o.criterion
    o.criterion = None
    with torch.no_grad():
        preds_o = o(img, mask, img_b, mask_b.clone())
    o.criterion = crit
    p2 = torch.cat([preds_o[1:, 0:1], preds_o[1:, 16:]], 1)                      # the base tile's novel-head logits [bg | novel]
    tt = F.interpolate(p2, size=(64, 64), mode='bilinear', align_corners=True).topk(2, dim=1).values
    near = ((tt[:, 0] - tt[:, 1]) <= 1e-5 * float(p2.abs().max())).numpy()
    dd = (mb_gpu.cpu() != mb_cpu).numpy()
    print('pseudo-labels: %d pixels differ, %d outside the 1e-5 margin, %d of %d pixels inside it' % (dd.sum(), (dd & ~near).sum(), near.sum(), near.size))
    assert int((dd & ~near).sum()) == 0 and near.sum() < 1e-3 * near.size
    assert int((mb_cpu > 15).sum()) > 0, 'no novel pseudo-label was written: the case checks nothing'
    for k, rt in (('seg_loss', 2e-4), ('orth_loss', 1e-4), ('total_loss', 2e-4)):
        print('%s: %.8g (oracle %.8g)' % (k, float(d[k].detach()), float(do[k].detach())))
        np.testing.assert_allclose(float(d[k].detach()), float(do[k].detach()), rtol=rt)
    check_grad(m.novel_emb.grad, o.novel_emb.grad, 5e-3, 'd_novel_emb')
    m.eval(); o.eval()
    with torch.no_grad():
        lg, lo = m(img.to(DEV)), o(img)
    assert tuple(lg.shape) == (1, 21, 8, 8)
    check(lg, lo, 1e-3, 'forward_all logits')
    label = fm.formula_mask(1, 64, 64, 21, 'wide/evmask', block=8, ignore_rows=4)
    pred, cm = confusion_of_batch(lg, label.to(DEV), num_classes=21, ignore_label=255)
    pred_o, cm_o = po.eval_confusion(lg.cpu(), label, 21, 255)
    up = F.interpolate(lg.cpu(), size=(64, 64), mode='bilinear', align_corners=True).topk(2, dim=1).values
    near = ((up[:, 0] - up[:, 1]) <= 1e-5 * float(lg.abs().max())).numpy()
    dp = pred.cpu().numpy() != pred_o
    assert int((dp & ~near).sum()) == 0 and near.sum() < 1e-3 * near.size
    keep = label.numpy() != 255
    assert np.array_equal(cm.cpu().numpy().astype(np.float64), po.confusion_matrix(label.numpy()[keep], pred.cpu().numpy()[keep], 21))
    if not dp.any():
        assert np.array_equal(cm.cpu().numpy().astype(np.float64), cm_o)


def test_swin_pop_20_classes_vs_same_box_oracle(hip):
    """Swin-T POP (128-channel head, padded from 96) at n_base=20: one train-mode forward + backward with the same DropPath draws on both sides and Dropout2d off;
    finite loss, loss dict to the G16 tolerances of test_swin_gpu.py (total / seg rtol 2e-4, orth 1e-4)."""
    from oracle import swin_oracle as so
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.networks.swin_pop import GFSS_Model
    m = fm.load_formula_weights(GFSS_Model(n_base=20, criterion=OrthLoss(255), backbone='swin-t', pretrained_model=None, compute_dtype=torch.float32)).to(DEV).train()
    o = fm.load_formula_weights(so.SwinPopOracle(20, criterion=po.OrthLossOracle(255))).train()
    drop = lambda i, B, p: None if p <= 0.0 else torch.tensor([0.0 if (7 * i + 3 * b) % 5 == 0 else 1.0 / (1.0 - p) for b in range(B)])
    m.backbone.drop_path_hook = drop
    o.drop_path_scale = drop
    m.decoder.dropout2d_hook = lambda B, C, p: torch.ones(B, C)
    o.dropout2d_scale = lambda B, C, p: None
    img = fm.formula_image(2, 96, 128, 'wide/swimg')
    mask = fm.formula_mask(2, 96, 128, 21, 'wide/swmask', block=8, ignore_rows=5)
    d = m(img.to(DEV), mask.to(DEV))
    d['total_loss'].backward()
    do = o(img, mask)
    assert bool(torch.isfinite(d['total_loss'])) and m.base_emb.grad is not None and bool(torch.isfinite(m.base_emb.grad).all())
    for k, rt in (('total_loss', 2e-4), ('seg_loss', 2e-4), ('orth_loss', 1e-4)):
        print('%s: %.8g (oracle %.8g)' % (k, float(d[k].detach()), float(do[k].detach())))
        np.testing.assert_allclose(float(d[k].detach()), float(do[k].detach()), rtol=rt)
