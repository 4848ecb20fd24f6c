"""The Lovasz-softmax term of include/segland_hip.h in torch float64, written from its definition (not from the kernels): the textbook sorted loss (Berman et al., batch-wide,
classes = "present"), the binned loss / table / histograms, the binned gradient with respect to the low-resolution logits, and `slack`, how far pixels that sit within
the float32 evaluation's reach of a bin edge can move that gradient.  Shared by test_lovasz_cpu.py and test_lovasz_gpu.py; no GPU, no library."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import formula as fm

NB = 1024
IGNORE = 255


def inputs(K, hw, HW, blank1=False):
    """the (low-resolution logits [2, K, h, w], label map [2, H, W]) of every Lovasz test at this shape"""
    preds = fm.sym('lov/p%d' % K, (2, K) + tuple(hw), 3.0)
    target = fm.formula_mask(2, HW[0], HW[1], K, tag='lov/m%d' % K, block=8, ignore_rows=5)
    if blank1:
        target = torch.cat([target[:1], torch.full_like(target[1:], IGNORE)])
    return preds, target


def upsample(logits, target, dtype=torch.float64):
    return F.interpolate(logits.to(dtype), size=tuple(target.shape[1:]), mode='bilinear', align_corners=True)


def errors(up, target):
    """(e, fg, p), each [N, K], at the N valid pixels of the batch: p = softmax, fg = [t == c], e = |fg - p| with the label's own error as (sum of the other
    exponentials) / (sum of all)"""
    K = up.shape[1]
    valid = (target != IGNORE) & (target >= 0) & (target < K)
    v = up.permute(0, 2, 3, 1)[valid]
    fg = F.one_hot(target[valid], K).bool()
    ex = (v - v.max(1, keepdim=True).values).exp()
    s = ex.sum(1, keepdim=True)
    p = ex / s
    u = ex.masked_fill(fg, 0).sum(1, keepdim=True) / s
    return torch.where(fg, u.expand_as(p), p), fg, p


def lovasz_grad(fg_sorted):
    """Berman et al., Alg. 1: the gradient of the Lovasz extension of the Jaccard loss with respect to the errors sorted in decreasing order"""
    g = fg_sorted.sum()
    inter = g - fg_sorted.cumsum(0)
    union = g + (1 - fg_sorted).cumsum(0)
    j = 1 - inter / union
    j[1:] = j[1:] - j[:-1].clone()
    return j


def exact_sorted(logits, target):
    """the textbook sorted Lovasz-softmax loss over the whole batch, mean over the present classes (0 without one), float64"""
    e, fg, _ = errors(upsample(logits, target), target)
    losses = []
    for c in range(e.shape[1]):
        f = fg[:, c].double()
        if f.sum() == 0:
            continue
        es, order = torch.sort(e[:, c], descending=True)
        losses.append(torch.dot(es, lovasz_grad(f[order])))
    return float(torch.stack(losses).mean()) if losses else 0.0


def bins_of(e, shift=0.0):
    return ((e + shift) * NB).floor().long().clamp(0, NB - 1)


def histogram(e, fg, shift=0.0):
    """int64 [K, NB, 2] = (foreground, background) counts per class and bin"""
    K = e.shape[1]
    j = bins_of(e, shift)
    idx = (torch.arange(K)[None, :] * NB + j) * 2 + (~fg).long()
    return torch.bincount(idx.reshape(-1), minlength=K * NB * 2).view(K, NB, 2)


def scan(hist):
    """(loss, table float64 [K, NB], n_present) from int64 histograms [K, NB, 2]: the definition's walk over the bins from the top"""
    hist = hist.to(torch.int64)
    Fh, Bh = hist[:, :, 0], hist[:, :, 1]
    G = Fh.sum(1, keepdim=True)
    f = Fh.flip(1).cumsum(1).flip(1)                      # bins >= j
    b = Bh.flip(1).cumsum(1).flip(1)
    present = G[:, 0] > 0
    J = 1 - (G - f).double() / (G + b).double().clamp(min=1)
    J = torch.where(present[:, None], J, torch.zeros_like(J))
    dJ = J - torch.cat([J[:, 1:], torch.zeros_like(J[:, :1])], 1)
    n_present = int(present.sum())
    centres = (torch.arange(NB, dtype=torch.float64) + 0.5) / NB
    loss = float((dJ * centres).sum(1)[present].sum() / n_present) if n_present else 0.0
    cnt = (Fh + Bh).double()
    table = torch.where((cnt > 0) & present[:, None], dJ / (cnt.clamp(min=1) * max(n_present, 1)), torch.zeros_like(dJ))
    return loss, table, n_present


def binned(logits, target):
    """(loss, table, hist) of the definition in float64"""
    e, fg, _ = errors(upsample(logits, target), target)
    hist = histogram(e, fg)
    loss, table, _ = scan(hist)
    return loss, table, hist


def pixel_grad(e, fg, p, table, shift=0.0):
    """[N, K]: p_k (q_k - sum_c p_c q_c) with q_c = (fg ? -1 : +1) table[c][bin(e_c + shift)]"""
    K = e.shape[1]
    q = table.to(p.dtype)[torch.arange(K)[None, :], bins_of(e, shift)] * torch.where(fg, -1.0, 1.0).to(p.dtype)
    return p * (q - (p * q).sum(1, keepdim=True))


def surrogate(up, target, table, bins=None):
    """a scalar of the upsampled logits `up` (any dtype) whose gradient is the Lovasz term's: sum over valid pixels and classes of q_c p_c with q held constant.  `bins`
    [N, K]: the bins to read the table at (default: those of `up`'s own errors)"""
    e, fg, p = errors(up, target)
    K = e.shape[1]
    j = bins_of(e.detach()) if bins is None else bins
    q = table.to(p.dtype)[torch.arange(K)[None, :], j] * torch.where(fg, -1.0, 1.0).to(p.dtype)
    return (q * p).sum()


def adjoint(pix, target, K, hw, dtype=torch.float64):
    """the transposed bilinear upsample applied to per-pixel values [N, K] at the valid pixels -> [B, K, h, w]"""
    valid = (target != IGNORE) & (target >= 0) & (target < K)
    full = torch.zeros(target.shape + (K,), dtype=dtype)
    full[valid] = pix.to(dtype)
    x = torch.zeros((target.shape[0], K) + tuple(hw), dtype=dtype, requires_grad=True)
    (upsample(x, target, dtype) * full.permute(0, 3, 1, 2)).sum().backward()
    return x.grad


def grad(logits, target, table, shift=0.0, dtype=torch.float64):
    """d lovasz / d logits [B, K, h, w] of the definition: the table is a constant, `shift` is added to every error before binning"""
    e, fg, p = errors(upsample(logits, target, dtype), target)
    return adjoint(pixel_grad(e, fg, p, table, shift), target, logits.shape[1], logits.shape[2:], dtype)


def margin(logits, target):
    """8 x the largest distance between the float32 and the float64 torch evaluation of e on the same inputs"""
    e64 = errors(upsample(logits, target), target)[0]
    e32 = errors(upsample(logits, target, torch.float32), target)[0]
    return 8.0 * float((e32.double() - e64).abs().max())


def near_edge(logits, target, m):
    """number of (pixel, class) pairs whose bin changes when the error moves by +-m, and the number of pairs"""
    e = errors(upsample(logits, target), target)[0]
    j = bins_of(e)
    return int(((bins_of(e, m) != j) | (bins_of(e, -m) != j)).sum()), e.numel()


def slack(logits, target, table, m=None):
    """[B, K, h, w] >= 0: D = max over shift in (+m, -m) of |pixel gradient(shift) - pixel gradient(0)| per pixel and channel, pushed through the transposed bilinear
    upsample (its weights are non-negative, so the result bounds what the bin-edge pixels can move in every output element).  From the reference alone."""
    m = margin(logits, target) if m is None else m
    e, fg, p = errors(upsample(logits, target), target)
    g0 = pixel_grad(e, fg, p, table)
    D = torch.maximum((pixel_grad(e, fg, p, table, m) - g0).abs(), (pixel_grad(e, fg, p, table, -m) - g0).abs())
    return adjoint(D, target, logits.shape[1], logits.shape[2:])


@functools.lru_cache(maxsize=None)
def case(K, hw, HW, blank1=False):
    """everything the tests share at one shape, computed once and never written to"""
    preds, target = inputs(K, hw, HW, blank1)
    loss, table, hist = binned(preds, target)
    m = margin(preds, target)
    ne, pairs = near_edge(preds, target, m)
    g = grad(preds, target, table)
    return dict(preds=preds, target=target, loss=loss, table=table, hist=hist, exact=exact_sorted(preds, target), m=m, near_edge=ne, pairs=pairs,
                grad=g, slack=slack(preds, target, table, m), n_present=int((hist[:, :, 0].sum(1) > 0).sum()),
                n_valid=int(((target != IGNORE) & (target >= 0) & (target < K)).sum()))
