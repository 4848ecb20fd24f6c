"""The sliding-window fusion of include/segland_hip.h (sl_slide_fuse) restated in torch, from its semantics alone: the window grid (side min(crop, L), offsets
min(i * stride, L - side)); per window, in (b, iy, ix) order with ix innermost, the bilinear upsampling with align_corners=True to the window size, softmax over the
classes ('prob') or nothing ('logit'), times the weight map (ones, or the tent min(y+1, ch-y) * min(x+1, cw-x)), `+=` into a [B,K,H,W] accumulator and a [H,W] weight map;
then the division and the argmax with the first maximum winning.  Runs in the dtype of the logits (float32: the reference, float64: the truth it is measured against) on
whatever device they are on."""
import torch
import torch.nn.functional as F

# the kernel-level cases of tests/test_slide_gpu.py: name -> (K, (H, W), crop, stride, (h, w), (offsets y, offsets x)); inputs fm.sym('slide/<name>', (2*ny*nx, K, h, w), 3.0)
CASES = {
    'a': (8, (40, 33), (16, 12), (8, 5), (5, 4), ([0, 8, 16, 24], [0, 5, 10, 15, 20, 21])),
    'b': (12, (72, 104), (32, 48), (21, 32), (4, 6), ([0, 21, 40], [0, 32, 56])),
    'c': (33, (40, 33), (24, 24), (24, 24), (3, 3), ([0, 16], [0, 9])),
    'd': (17, (9, 1), (4, 4), (3, 3), (2, 1), ([0, 3, 5], [0])),
    'e': (16, (33, 40), (64, 16), (7, 16), (5, 2), ([0], [0, 16, 24])),
    'f': (8, (30, 30), (16, 16), (1, 15), (2, 2), (list(range(15)), [0, 14])),
}
BATCH = 2


def grid(L, crop, stride):
    """(side, offsets) along one side, from the formula."""
    assert L >= 1 and crop >= 1 and 1 <= stride <= crop
    side = min(crop, L)
    n = max(L - side + stride - 1, 0) // stride + 1
    return side, [min(i * stride, L - side) for i in range(n)]


def weight_map(ch, cw, blend, dtype, device):
    if blend == 'uniform':
        return torch.ones((ch, cw), dtype=dtype, device=device)
    assert blend == 'tent'
    y = torch.arange(ch, device=device)
    x = torch.arange(cw, device=device)
    return (torch.minimum(y + 1, ch - y)[:, None] * torch.minimum(x + 1, cw - x)[None, :]).to(dtype)


def fuse(logits, B, size, crop, stride, mode='prob', blend='uniform'):
    """logits [B*ny*nx,K,h,w] -> (labels int64 [B,H,W], fused [B,K,H,W]) in the logits' dtype."""
    H, W = size
    ch, ys = grid(H, crop[0], stride[0])
    cw, xs = grid(W, crop[1], stride[1])
    assert logits.shape[0] == B * len(ys) * len(xs)
    K = logits.shape[1]
    wmap = weight_map(ch, cw, blend, logits.dtype, logits.device)
    acc = torch.zeros((B, K, H, W), dtype=logits.dtype, device=logits.device)
    den = torch.zeros((H, W), dtype=logits.dtype, device=logits.device)
    for b in range(B):
        for iy, y1 in enumerate(ys):
            for ix, x1 in enumerate(xs):
                n = (b * len(ys) + iy) * len(xs) + ix
                t = F.interpolate(logits[n:n + 1], size=(ch, cw), mode='bilinear', align_corners=True)[0]
                if mode == 'prob':
                    t = torch.softmax(t, dim=0)
                acc[b, :, y1:y1 + ch, x1:x1 + cw] += wmap * t
                if b == 0:
                    den[y1:y1 + ch, x1:x1 + cw] += wmap
    fused = acc / den
    return fused.argmax(dim=1), fused

