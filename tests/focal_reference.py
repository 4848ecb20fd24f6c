"""The focal criterion of include/segland_hip.h in torch, for the tests of the fused kernels: float64 is the reference, float32 the yardstick for its error.

    up = F.interpolate(logits, (H, W), bilinear, align_corners=True);  logp = log_softmax(up);  u = -expm1(logp_t)  (= 1 - p_t, no cancellation);  mod = u^gamma
    num0 = -sum_k c_k logp_k,  c_k = (1 - eps) w_t [k == t] + (eps / K) w_k;  den = w_t;  loss = sum mod * num0 / sum den  over the valid pixels

`gamma == 0` stands for mod == 1 (the cross-entropy itself).  closed_form_grad is the gradient formula of the header on a matrix of per-pixel logits; kernel_u replays the
kernels' own float32 evaluation of u (exponentials summed in index order, the label's skipped) in numpy, to count the pixels where it saturates."""
import numpy as np
import torch
import torch.nn.functional as F


def valid_mask(target, K, ignore=255):
    return (target != ignore) & (target >= 0) & (target < K)


def pixel_terms(v, t, gamma, w=None, eps=0.0):
    """(mod, num0, den) of the pixels v [N, K] with labels t [N] (all valid), in v's dtype"""
    K = v.shape[1]
    w = torch.ones(K, dtype=v.dtype) if w is None else w.to(v.dtype)
    logp = v.log_softmax(1)
    logpt = logp.gather(1, t[:, None])[:, 0]
    u = -torch.expm1(logpt)
    mod = torch.ones_like(u) if gamma == 0 else u ** gamma
    num0 = -((1.0 - eps) * w[t] * logpt + (eps / K) * (logp * w).sum(1))
    return mod, num0, w[t]


def focal_loss(up, target, gamma, w=None, eps=0.0, ignore=255):
    """(loss, weight sum) on upsampled logits `up` [B, K, H, W]"""
    K = up.shape[1]
    valid = valid_mask(target, K, ignore)
    v = up.permute(0, 2, 3, 1)[valid]
    mod, num0, den = pixel_terms(v, target[valid], gamma, w, eps)
    return (mod * num0).sum() / den.sum(), den.sum()


def upsample(logits, HW):
    return F.interpolate(logits, size=tuple(HW), mode='bilinear', align_corners=True)


def focal_with_grad(logits, target, HW, gamma, w, eps, dtype, gs=1.0, extra=None):
    """(loss, weight sum, d (gs * (loss + extra(up))) / d logits) in `dtype`; extra: an added term of the upsampled logits (the Dice term of the hybrid tests)"""
    pr = logits.to(dtype).clone().requires_grad_(True)
    up = upsample(pr, HW)
    loss, wsum = focal_loss(up, target, gamma, w, eps)
    total = loss if extra is None else loss + extra(up)
    (total * gs).backward()
    return float(loss.detach()), float(wsum), pr.grad.numpy()


def closed_form_grad(v, t, gamma, w=None, eps=0.0):
    """d (sum of the pixel numerators) / d v by the header's formula: mod * ceform + beta * (p - onehot), beta = gamma * num0 * u^(gamma - 1) * p_t (0 where u == 0)"""
    K = v.shape[1]
    wv = torch.ones(K, dtype=v.dtype) if w is None else w.to(v.dtype)
    mod, num0, wt = pixel_terms(v, t, gamma, w, eps)
    p = v.softmax(1)
    onehot = F.one_hot(t, K).to(v.dtype)
    u = -torch.expm1(v.log_softmax(1).gather(1, t[:, None])[:, 0])
    ct = (1.0 - eps) * wt + (eps / K) * wv.sum()
    ceform = p * ct[:, None] - ((1.0 - eps) * wt[:, None] * onehot + (eps / K) * wv[None, :])
    modu = torch.where(u > 0, u ** (gamma - 1.0), torch.zeros_like(u))
    beta = gamma * num0 * modu * p.gather(1, t[:, None])[:, 0]
    return mod[:, None] * ceform + beta[:, None] * (p - onehot)


def kernel_u(up32, target, ignore=255):
    """float32 numpy replay of the kernels' u on upsampled float32 logits [B, K, H, W]: u of every valid pixel, in pixel order"""
    K = up32.shape[1]
    valid = valid_mask(target, K, ignore)
    v = up32.permute(0, 2, 3, 1)[valid].numpy().astype(np.float32)
    t = target[valid].numpy()
    e = np.exp(v - v.max(1, keepdims=True), dtype=np.float32)
    s = np.zeros(len(v), np.float32)
    so = np.zeros(len(v), np.float32)
    for k in range(K):                                   # index order, float32 partial sums
        s = (s + e[:, k]).astype(np.float32)
        so = np.where(t == k, so, (so + e[:, k]).astype(np.float32))
    return (so / s).astype(np.float32)
