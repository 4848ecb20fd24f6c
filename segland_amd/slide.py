"""Sliding-window inference of one model: the scene is cut into overlapping windows of the model's own crop size, the windows are plain forwards, and their fusion on the
scene grid is ONE kernel (ops.slide_fuse -> sl_slide_fuse: per covering window the bilinear upsampling with align_corners=True to the crop, optional softmax, uniform or
tent weights, weighted mean and argmax; no per-window map and no accumulator is written).  Model-agnostic: `model` is any callable image [N,3,ch,cw] -> logits [N,K,h,w].

The window grid along one side of length L with crop c and stride s (1 <= s <= c): window side c' = min(c, L), n = max(L - c' + s - 1, 0) // s + 1 windows, window i at
offset min(i * s, L - c') -- the last window is shifted back to end at the border.  sl_slide_windows is the same count in C (asserted over a sweep)."""
import torch

from . import ops


def window_grid(L, crop, stride):
    """(side, offsets) of the windows along one side; ValueError unless L, crop >= 1 and 1 <= stride <= crop (a stride above the crop as given would leave holes)."""
    L, crop, stride = int(L), int(crop), int(stride)
    if L < 1 or crop < 1:
        raise ValueError('slide: side %d and crop %d must be at least 1' % (L, crop))
    if not 1 <= stride <= crop:
        raise ValueError('slide: stride %d outside [1, crop %d]' % (stride, crop))
    side = min(crop, L)
    n = max(L - side + stride - 1, 0) // stride + 1
    return side, [min(i * stride, L - side) for i in range(n)]


def parse_pair(text):
    """'512,512' -> (512, 512); one number stands for both sides; '' -> None (the flag was not given)."""
    items = [t.strip() for t in str(text).split(',') if t.strip()]
    if not items:
        return None
    if len(items) > 2:
        raise ValueError('slide: %r is not H,W' % (text,))
    pair = tuple(int(t) for t in items)
    pair = pair * 2 if len(pair) == 1 else pair
    if min(pair) < 1:
        raise ValueError('slide: %r holds a side below 1' % (text,))
    return pair


def is_on(crop):
    """Sliding runs when a crop is given; otherwise the whole-image pipeline runs as it is."""
    return bool(crop)


def default_stride(crop):
    """Two thirds of the crop, rounded down, at least 1."""
    return tuple(max(1, (2 * c) // 3) for c in crop)


def driver_geometry(crop_text, stride_text, align=32):
    """(crop, stride) of the evaluation drivers' --slide-crop / --slide-stride, or (None, None) when sliding is off.  Crop sides given on the command line must be
    multiples of `align` (the alignment tta.py rounds its views to, for the same reason: the backbone's strides and the pyramid bins); the functions here take any size."""
    crop = parse_pair(crop_text)
    if not is_on(crop):
        return None, None
    if any(c % align for c in crop):
        raise ValueError('--slide-crop %d,%d: both sides must be multiples of %d' % (crop[0], crop[1], align))
    stride = parse_pair(stride_text) or default_stride(crop)
    for s, c in zip(stride, crop):
        if not 1 <= s <= c:
            raise ValueError('--slide-stride %d,%d outside [1, crop %d,%d]' % (stride[0], stride[1], crop[0], crop[1]))
    return crop, stride


def windows(image, crop, stride):
    """The windows of image [B,3,H,W] as one batch [B*ny*nx,3,ch,cw], window (b, iy, ix) at index (b*ny + iy)*nx + ix.  Plain slicing: not the hot path."""
    B, H, W = image.shape[0], image.shape[-2], image.shape[-1]
    ch, ys = window_grid(H, crop[0], stride[0])
    cw, xs = window_grid(W, crop[1], stride[1])
    out = image.new_empty((B * len(ys) * len(xs),) + tuple(image.shape[1:-2]) + (ch, cw))
    out5 = out.view((B, len(ys) * len(xs)) + tuple(out.shape[1:]))
    for iy, y in enumerate(ys):
        for ix, x in enumerate(xs):
            out5[:, iy * len(xs) + ix] = image[..., y:y + ch, x:x + cw]
    return out


def predict(model, image, crop, stride, mode='prob', blend='uniform', want_map=False, batch=0):
    """(labels uint8 [B,H,W], fused map float [B,K,H,W] or None) on the grid of `image`: the windows are forwarded in chunks of `batch` (0: all at once) under no_grad,
    every chunk's logits go into one preallocated [N,K,h,w] tensor, then one call of ops.slide_fuse."""
    B, H, W = image.shape[0], image.shape[-2], image.shape[-1]
    win = windows(image, crop, stride)
    N = win.shape[0]
    step = N if int(batch) <= 0 else int(batch)
    logits = None
    with torch.no_grad():
        for i in range(0, N, step):
            out = model(win[i:i + step]).float()
            if logits is None:
                logits = out.new_empty((N,) + tuple(out.shape[1:]))
            logits[i:i + step] = out
    return ops.slide_fuse(logits, B, (H, W), crop, stride, mode=mode, blend=blend, want_map=want_map)
