"""Online hard-pixel mining (OHEM, bootstrapped cross-entropy) as include/segland_hip.h defines it, restated in torch from that definition alone and run on the CPU:

    up = F.interpolate(logits, (H, W), bilinear, align_corners=True);  p = softmax(up)[label] on the valid pixels (label != ignore and inside [0, K)), n of them
    k = min(min_kept, n);  q = sort(p)[k - 1];  theta = max(thresh, q);  kept = valid & (p <= theta);  mined = target on kept pixels, ignore elsewhere (n == 0: target)

and the head's criterion, torch's cross_entropy or the Dice definition of tests/test_dice_loss_gpu.py, on (up, mined).  Shared by tests/test_ohem_cpu.py and
tests/test_ohem_gpu.py; runs in the dtype of the logits (float32: the reference, float64: what its own error is measured against)."""
import torch
import torch.nn.functional as F

from oracle import formula as fm

# (K, (h, w), (H, W)): both per-thread widths of the kernels, a ragged map, the identity scale
SHAPES = [(8, (8, 8), (64, 64)), (12, (9, 7), (40, 33)), (33, (8, 8), (64, 64)), (33, (8, 8), (8, 8))]
GAP = 1e-5                       # a case is valid only if no probability lies this close to theta (other than q and its exact ties)


def upsample(logits, HW):
    return F.interpolate(logits, size=tuple(HW), mode='bilinear', align_corners=True)


def true_class_prob(logits, target, ignore=255):
    """(p [B, H, W] with 2.0 on the pixels that are not valid, valid [B, H, W] bool)"""
    K = logits.shape[1]
    valid = (target != ignore) & (target >= 0) & (target < K)
    p = upsample(logits, target.shape[1:]).softmax(1).gather(1, target.masked_fill(~valid, 0)[:, None])[:, 0]
    return torch.where(valid, p, torch.full_like(p, 2.0)), valid


def mine(logits, target, thresh, min_kept, ignore=255):
    """The definition.  gap: the distance from theta of the nearest valid probability that is neither theta's own q nor an exact tie of it."""
    p, valid = true_class_prob(logits, target, ignore)
    pv = p[valid]
    n = int(pv.numel())
    th = torch.tensor(float(thresh), dtype=p.dtype)
    if n == 0:
        return dict(p=p, valid=valid, n=0, k=0, q=None, theta=float(th), kept=valid.clone(), n_kept=0, mined=target.clone(), gap=float('inf'), ties=0, binds=False)
    k = min(int(min_kept), n)
    q = pv.sort().values[k - 1]
    theta = torch.maximum(th, q)
    kept = valid & (p <= theta)
    mined = torch.where(kept, target, torch.full_like(target, ignore))
    binds = bool(q > th)                                # theta = q: min_kept decides, not the threshold
    others = pv[pv != q] if binds else pv
    gap = float((others - theta).abs().min()) if others.numel() else float('inf')
    return dict(p=p, valid=valid, n=n, k=k, q=float(q), theta=float(theta), kept=kept, n_kept=int(kept.sum()), mined=mined, gap=gap, ties=int((pv == q).sum()), binds=binds)


def dice(up, target, w, s, ignore=255):
    """multiclass soft Dice with softmax (tests/test_dice_loss_gpu.torch_dice): sum over classes, each scaled by w, mean over samples; ignored pixels enter no sum"""
    K = up.shape[1]
    p = up.softmax(1)
    valid = target != ignore
    oh = F.one_hot(target.masked_fill(~valid, 0), K).permute(0, 3, 1, 2).to(up.dtype) * valid[:, None]
    pm = p * valid[:, None]
    I, P, T = (pm * oh).sum((2, 3)), pm.sum((2, 3)), oh.sum((2, 3))
    d = 1 - (2 * I + s) / (P + T + s)
    return (d * (w.to(up.dtype) if w is not None else 1)).sum(1).mean()


def head_loss(logits, target, thresh, min_kept, w=None, eps=0.0, lam=0.0, s=1.0, ignore=255):
    """(seg loss of one head = cross-entropy + lam * Dice on the mined map, Dice term, the mining record); thresh None: no mining.  Differentiable in `logits`; the kept
    set is a constant."""
    with torch.no_grad():
        rec = mine(logits.detach(), target, thresh, min_kept, ignore) if thresh is not None else dict(mined=target)
    tgt = rec['mined']
    tgt = tgt.masked_fill((tgt < 0) | (tgt >= logits.shape[1]), ignore)            # labels outside [0, K) count as ignored
    up = upsample(logits, target.shape[1:])
    ce = F.cross_entropy(up, tgt, weight=None if w is None else w.to(up.dtype), ignore_index=ignore, label_smoothing=eps)
    if not bool((tgt != ignore).any()):
        ce = up.sum() * 0.0                                                          # torch gives nan for an empty mean; the comparison never uses this case's value
    d = dice(up, tgt, w, s, ignore) if lam > 0.0 else None
    return (ce + lam * d if d is not None else ce), d, rec


def random_logits(tag, K, hw, salt=0, bound=3.5):
    """uniform in [-bound, bound] (standard deviation ~2): most true-class probabilities are small, the threshold decides"""
    return fm.sym('ohem/%s/p%d' % (tag, K), (2, K) + tuple(hw), bound, salt=salt)


def labels(tag, K, HW, salt=0):
    """[2, H, W] labels in [0, K), rows 0..4 of sample 0 ignored"""
    return fm.formula_mask(2, HW[0], HW[1], K, tag='ohem/%s/m%d/%d' % (tag, K, salt), block=8, ignore_rows=min(5, HW[0] - 1))


def mostly_right_logits(tag, K, hw, target, salt=0, boost=6.0, bound=1.5):
    """random logits plus `boost` at the label of the nearest pixel of the label map for every coarse cell: most pixels are confidently right, min_kept decides"""
    lg = fm.sym('ohem/%s/r%d' % (tag, K), (2, K) + tuple(hw), bound, salt=salt)
    H, W = target.shape[1:]
    ys = torch.round(torch.arange(hw[0], dtype=torch.float64) * ((H - 1) / max(hw[0] - 1, 1))).long()
    xs = torch.round(torch.arange(hw[1], dtype=torch.float64) * ((W - 1) / max(hw[1] - 1, 1))).long()
    near = target[:, ys][:, :, xs]
    ok = (near >= 0) & (near < K)
    return lg + boost * F.one_hot(near.masked_fill(~ok, 0), K).permute(0, 3, 1, 2).float() * ok[:, None]
