"""The contract of sl_augment_batch_ex (include/segland_hip.h) restated in numpy float64: bilinear taps and nearest label indices in exact integers, the colour jitter, and the
crop / pad / flip / rot90 / normalise tail.  Nothing here imports the package: the tests compare the product against this file, and this file against torch on the CPU where the
conventions coincide.  Every function works on ONE tile."""
import numpy as np


def scaled_size(n, s):
    return max(1, int(n * s + 0.5))


def taps(P, S, Ss):
    """(p0, p1, frac float64, nearest label index) of the rescaled indices P on an axis S -> Ss."""
    P = np.asarray(P, dtype=np.int64)
    n = np.maximum((2 * P + 1) * S - Ss, 0)
    d = 2 * Ss
    p0 = n // d
    p1 = np.minimum(p0 + 1, S - 1)
    frac = (n - p0 * d).astype(np.float64) / float(d)
    pl = np.minimum(((2 * P + 1) * S) // d, S - 1)
    return p0, p1, frac, pl


def tie(P, S, Ss):
    """True where the centre of rescaled pixel P falls exactly between two source pixels."""
    P = np.asarray(P, dtype=np.int64)
    return ((2 * P + 1) * S) % (2 * Ss) == 0


def resample(img, Hs, Ws):
    """uint8 / float [H,W,C] -> float64 [Hs,Ws,C], bilinear, align_corners=False."""
    H, W = img.shape[:2]
    v = img.astype(np.float64)
    y0, y1, fy, _ = taps(np.arange(Hs), H, Hs)
    x0, x1, fx, _ = taps(np.arange(Ws), W, Ws)
    fx = fx[None, :, None]
    fy = fy[:, None, None]
    a = v[y0][:, x0] * (1.0 - fx) + v[y0][:, x1] * fx
    b = v[y1][:, x0] * (1.0 - fx) + v[y1][:, x1] * fx
    return a * (1.0 - fy) + b * fy


def resample_label(lbl, Hs, Ws):
    H, W = lbl.shape
    ly = taps(np.arange(Hs), H, Hs)[3]
    lx = taps(np.arange(Ws), W, Ws)[3]
    return lbl[ly][:, lx]


def jitter(v, alpha, beta, sigma):
    """v float64 [...,3] in R, G, B order, values in [0, 255]."""
    v = np.clip(v * alpha + beta * 255.0, 0.0, 255.0)
    g = (0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2])[..., None]
    return np.clip(g + (v - g) * sigma, 0.0, 255.0)


def prepare(img, lbl, draw, crop, mean, std, ignore_label=255, lut=None, resampled=None):
    """One tile through the whole contract.  img uint8 [H,W,3], lbl uint8 [H,W] or None, draw = (h_off, w_off, flip, k, Hs, Ws, jitter, alpha, beta, sigma, ...)
    -> (float64 [3,ch,cw], int64 [ch,cw] or None, bool [ch,cw]: True where the output pixel is padding).  resampled: resample(img, Hs, Ws) computed before (it does not
    depend on the rest of the draw)."""
    h_off, w_off, flip, k, Hs, Ws, jit, alpha, beta, sigma = draw[:10]
    ch, cw = crop
    v = resample(img, Hs, Ws) if resampled is None else resampled
    assert v.shape == (Hs, Ws, 3)
    if jit:                                               # per pixel: only the window the crop keeps needs it
        v = v.copy()
        win = (slice(h_off, h_off + ch), slice(w_off, w_off + cw))
        v[win] = jitter(v[win], alpha, beta, sigma)
    canvas = np.zeros((h_off + ch, w_off + cw, 3))
    pad = np.ones((h_off + ch, w_off + cw), dtype=bool)
    lab = np.full((h_off + ch, w_off + cw), ignore_label, dtype=np.int64)
    hh, ww = min(Hs, h_off + ch), min(Ws, w_off + cw)
    canvas[:hh, :ww] = v[:hh, :ww]
    pad[:hh, :ww] = False
    if lbl is not None:
        l = resample_label(lbl, Hs, Ws).astype(np.int64)
        lab[:hh, :ww] = (np.asarray(lut, dtype=np.int64)[l] if lut is not None else l)[:hh, :ww]
    out = []
    for m in (canvas, lab, pad):
        m = m[h_off:h_off + ch, w_off:w_off + cw]
        if flip:
            m = np.flip(m, axis=1)
        out.append(np.rot90(m, k, (0, 1)))
    image, lab, pad = out
    image = image[:, :, ::-1] / 255.0
    image = (image - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    return np.ascontiguousarray(image.transpose(2, 0, 1)), (None if lbl is None else np.ascontiguousarray(lab)), np.ascontiguousarray(pad)


def source_rows_brute(H, Hs, h_off, ch):
    """(row0, rows) of the source rows the taps and the labels of crop rows [h_off, min(h_off + ch, Hs)) read, from the tap lists themselves."""
    y0, y1, _, ly = taps(np.arange(h_off, min(h_off + ch, Hs)), H, Hs)
    lo, hi = int(min(y0.min(), ly.min())), int(max(y1.max(), ly.max()))
    return lo, hi - lo + 1
