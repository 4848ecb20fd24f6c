"""Multi-scale + flip test-time augmentation of one model: the views are plain forwards at resized / mirrored images, their fusion on the label grid is ONE kernel
(ops.tta_fuse -> sl_tta_fuse: bilinear upsampling with align_corners=True, optional softmax, un-flip, weighted mean and argmax; no per-view H x W map is written).
Model-agnostic: `model` is any callable image [B,3,H,W] -> logits [B,K,h,w]."""
import math

import torch
import torch.nn.functional as F

from . import ops
from ._lib import SL_TTA_MAX_VIEWS


def parse_scales(text):
    """'0.75,1.0,1.25' -> (0.75, 1.0, 1.25); ValueError on an empty list, a non-positive or a non-finite value."""
    items = [t.strip() for t in str(text).split(',') if t.strip()]
    if not items:
        raise ValueError('tta: empty list of scales: %r' % (text,))
    scales = tuple(float(t) for t in items)
    for s in scales:
        if not (math.isfinite(s) and s > 0):
            raise ValueError('tta: scale %r is not a finite value > 0' % (s,))
    return scales


def scaled_size(H, W, s, align):
    """Image size of the view at scale s: (H, W) itself at s == 1.0, else each side rounded to the nearest multiple of `align` (at least one)."""
    if s == 1.0:
        return (H, W)
    return tuple(max(align, int(math.floor(x * s / align + 0.5)) * align) for x in (H, W))


def is_on(scales, flip):
    """More than one scale, a scale other than 1.0, or flip: otherwise the single-view pipeline runs as it is."""
    return bool(flip) or len(scales) != 1 or scales[0] != 1.0


def view_sizes(H, W, scales, align=32):
    return [scaled_size(H, W, s, align) for s in scales]


def views(model, image, scales, flip, align=32):
    """[(logits float [B,K,h,w], flip bits, weight 1.0), ...] per scale in list order, the plain view first and, with `flip`, the horizontally mirrored one after it."""
    if len(scales) * (2 if flip else 1) > SL_TTA_MAX_VIEWS:
        raise ValueError('tta: %d scales%s make more than %d views' % (len(scales), ' with flip' if flip else '', SL_TTA_MAX_VIEWS))
    H, W = image.shape[-2:]
    out = []
    with torch.no_grad():
        for s in scales:
            im = image if s == 1.0 else F.interpolate(image, scaled_size(H, W, s, align), mode='bilinear', align_corners=False)
            out.append((model(im).float().contiguous(), 0, 1.0))
            if flip:
                out.append((model(im.flip(-1)).float().contiguous(), 1, 1.0))
    return out


def predict(model, image, size, scales=(1.0,), flip=False, mode='prob', want_map=False, align=32):
    """(labels uint8 [B,H,W], fused map float [B,K,H,W] or None) at `size` from the views above."""
    return ops.tta_fuse(views(model, image, scales, flip, align), size, mode=mode, want_map=want_map)
