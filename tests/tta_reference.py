"""The test-time-augmentation fusion of include/segland_hip.h (sl_tta_fuse) restated in torch, from its semantics alone: per view the bilinear upsampling with
align_corners=True, un-flipped by torch.flip; softmax over the classes ('prob') or nothing ('logit'); the weighted sum in list order with term 0 starting it, divided by
the weight sum taken in the same order; argmax with the first maximum winning.  Runs in the dtype of the views (float32: the reference, float64: the truth it is
measured against) on whatever device they are on."""
import torch
import torch.nn.functional as F

# the kernel-level cases of tests/test_tta_gpu.py: name -> (K, (H, W), [(h, w, flip, weight), ...]), inputs fm.sym('tta/<name>/<i>', (2, K, h, w), 3.0)
CASES = {
    'a': (8, (40, 33), [(9, 7, 0, 1.0), (9, 7, 1, 1.0)]),
    'b': (12, (72, 104), [(9, 13, 0, 1.0), (9, 13, 1, 1.0), (5, 7, 0, 0.5), (5, 7, 1, 0.5), (13, 19, 0, 1.0), (13, 19, 3, 1.0)]),
    'c': (33, (40, 33), [(5, 5, 0, 1.0), (7, 6, 1, 2.0), (9, 7, 2, 1.0)]),
    'd': (17, (1, 1), [(3, 4, 0, 1.0), (1, 1, 1, 1.0)]),
    'e': (16, (33, 40), [(5, 5, 0, 1.0), (40, 33, 1, 1.0)]),
}


def flip_dims(flip):
    return [d for bit, d in ((1, -1), (2, -2)) if flip & bit]


def unflipped(logits, size, flip):
    up = F.interpolate(logits, size=tuple(size), mode='bilinear', align_corners=True)
    dims = flip_dims(flip)
    return torch.flip(up, dims) if dims else up


def fuse(views, size, mode='prob'):
    """views: [(logits [B,K,h,w], flip, weight), ...] -> (labels int64 [B,H,W], fused [B,K,H,W]) in the views' dtype."""
    acc, wsum = None, None
    for logits, flip, weight in views:
        t = unflipped(logits, size, flip)
        if mode == 'prob':
            t = torch.softmax(t, dim=1)
        w = torch.tensor(float(weight), dtype=logits.dtype, device=logits.device)
        acc = w * t if acc is None else acc + w * t
        wsum = w if wsum is None else wsum + w
    fused = acc / wsum
    return fused.argmax(dim=1), fused

