"""The contract of sl_augment_batch_geo (include/segland_hip.h) restated in numpy: rotation about the crop centre, separable Gaussian blur with a reflect-101 border, then the
jitter and the tail of sl_augment_batch_ex.  Nothing here imports the package.  `prepare` works on ONE tile and evaluates the value chain in float64 (the yardstick) or, with
dtype=np.float32, in the kernel's own precision -- the coordinates are double in both, as in the kernel -- so that the distance between the two gives the tests their tolerance.
The near-tie mask marks the pixels where a coordinate sits within 1e-9 of a rounding boundary: there a last-bit difference may move a label or the inside test, and the tests
compare nothing."""
import math

import numpy as np

import aug_reference as ar

TIE_EPS = 1e-9


def blur_weights(K):
    """Half kernel (centre first) of the K-tap Gaussian with OpenCV's sigma rule, computed in float64 and rounded to float32 as the record stores it; returned as float64."""
    R = (K - 1) // 2
    sigma = 0.3 * ((K - 1) * 0.5 - 1.0) + 0.8
    g = np.exp(-np.arange(R + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return (g / (g[0] + 2.0 * g[1:].sum())).astype(np.float32).astype(np.float64)


def angle_draw(h_off, w_off, flip, k, Hs, Ws, triple, H, angle=None, blur_k=0):
    """The 16 fields of a GeoDraw as a plain tuple; angle in degrees or None (rotate = 0), triple (alpha, beta, sigma) or None (jitter off)."""
    a, b, s = triple or (1.0, 0.0, 1.0)
    rot = angle is not None
    t = math.radians(angle) if rot else 0.0
    return (h_off, w_off, flip, k, Hs, Ws, int(triple is not None), a, b, s, H, 0, int(rot), math.cos(t) if rot else 1.0, math.sin(t) if rot else 0.0, blur_k)


def coords(draw, crop):
    """(U, V) float64 [ch, cw] of step 2 for a rotated draw, in the kernel's order of operations."""
    h_off, w_off = draw[0], draw[1]
    cos_t, sin_t = draw[13], draw[14]
    ch, cw = crop
    hx, hy = 0.5 * cw, 0.5 * ch
    dx = (np.arange(cw, dtype=np.float64) - hx)[None, :]
    dy = (np.arange(ch, dtype=np.float64) - hy)[:, None]
    return w_off + (hx + (cos_t * dx - sin_t * dy)), h_off + (hy + (sin_t * dx + cos_t * dy))


def real_taps(P, S, Ss):
    """(p0, p1, frac float64, nearest label index, s) of real rescaled coordinates P on an axis S -> Ss (step 4)."""
    s = ((P + 0.5) * float(S)) / float(Ss) - 0.5
    sc = np.clip(s, 0.0, S - 1.0)
    p0 = np.floor(sc).astype(np.int64)
    p1 = np.minimum(p0 + 1, S - 1)
    pl = np.clip(np.floor(s + 0.5), 0, S - 1).astype(np.int64)
    return p0, p1, sc - p0, pl, s


def _near_integer(v):
    return np.abs(v - np.round(v)) <= TIE_EPS


def sample(img, lbl, draw, crop, dtype=np.float64):
    """Steps 2-4 on the (r, c) grid: (R, G, B [ch,cw,3] of `dtype` with 0 at the padding, raw label int64 [ch,cw] (garbage at the padding), inside bool, near-tie bool,
    (rows, cols) int64 of every source index read by a tap or a label of an inside pixel)."""
    h_off, w_off, _, _, Hs, Ws = draw[:6]
    H, W = img.shape[:2]
    ch, cw = crop
    if not draw[12]:
        Y, X = h_off + np.arange(ch), w_off + np.arange(cw)
        y0, y1, fy, ly = ar.taps(Y, H, Hs)
        x0, x1, fx, lx = ar.taps(X, W, Ws)
        inside = (Y < Hs)[:, None] & (X < Ws)[None, :]
        y0, y1, ly = (np.minimum(a, H - 1) for a in (y0, y1, ly))              # positions beyond the rescaled tile are padding: keep their indices readable
        x0, x1, lx = (np.minimum(a, W - 1) for a in (x0, x1, lx))
        y0, y1, fy, ly = (np.broadcast_to(a[:, None], (ch, cw)) for a in (y0, y1, fy, ly))
        x0, x1, fx, lx = (np.broadcast_to(a[None, :], (ch, cw)) for a in (x0, x1, fx, lx))
        tie = np.zeros((ch, cw), dtype=bool)
    else:
        U, V = coords(draw, crop)
        iu, iv = np.floor(U + 0.5), np.floor(V + 0.5)
        inside = (iu >= 0) & (iu < Ws) & (iv >= 0) & (iv < Hs)
        y0, y1, fy, ly, sy = real_taps(V, H, Hs)
        x0, x1, fx, lx, sx = real_taps(U, W, Ws)
        tie = _near_integer(U + 0.5) | _near_integer(V + 0.5) | _near_integer(sx + 0.5) | _near_integer(sy + 0.5)
    v = img.astype(dtype)
    fx, fy = fx.astype(dtype)[..., None], fy.astype(dtype)[..., None]           # fx = (float)(sxc - x0) in the kernel
    one = dtype(1.0)
    a = v[y0, x0] * (one - fx) + v[y0, x1] * fx
    b = v[y1, x0] * (one - fx) + v[y1, x1] * fx
    p = a * (one - fy) + b * fy
    p[~inside] = 0
    lab = lbl[ly, lx].astype(np.int64) if lbl is not None else np.zeros((ch, cw), dtype=np.int64)
    rows = np.concatenate([y0[inside], y1[inside], ly[inside]])
    cols = np.concatenate([x0[inside], x1[inside], lx[inside]])
    return p, lab, inside, tie, (rows, cols)


def blur(p, K, dtype=np.float64):
    """Step 5 on a [h,w,C] crop-frame image: along the columns first, then along the rows, reflect-101 border, centre tap first and the pairs at distance i summed before they
    are weighted."""
    R = (K - 1) // 2
    w = blur_weights(K).astype(dtype)
    h, wd = p.shape[:2]
    q = np.pad(p.astype(dtype), ((0, 0), (R, R), (0, 0)), mode='reflect')
    acc = w[0] * q[:, R:R + wd]
    for i in range(1, R + 1):
        acc = acc + w[i] * (q[:, R - i:R - i + wd] + q[:, R + i:R + i + wd])
    q = np.pad(acc, ((R, R), (0, 0), (0, 0)), mode='reflect')
    out = w[0] * q[R:R + h]
    for i in range(1, R + 1):
        out = out + w[i] * (q[R - i:R - i + h] + q[R + i:R + i + h])
    return out


def jitter(v, alpha, beta, sigma, dtype=np.float64):
    """Step 5 of sl_augment_batch_ex in `dtype` (float64: aug_reference.jitter)."""
    if dtype == np.float64:
        return ar.jitter(v, alpha, beta, sigma)
    f = np.float32
    v = np.clip(v * f(alpha) + f(beta * 255.0), f(0), f(255))
    g = ((f(0.299) * v[..., 0] + f(0.587) * v[..., 1]) + f(0.114) * v[..., 2])[..., None]
    return np.clip(g + (v - g) * f(sigma), f(0), f(255))


def prepare(img, lbl, draw, crop, mean, std, ignore_label=255, lut=None, dtype=np.float64):
    """One tile through the whole contract: (image [3,ch,cw] float64 -- rounded through float32 where the kernel rounds when dtype is float32 --, label int64 [ch,cw] or None,
    padding mask, near-tie mask), all on the output grid."""
    flip, k, jit, alpha, beta, sigma, blur_k = draw[2], draw[3], draw[6], draw[7], draw[8], draw[9], draw[15]
    p, lab, inside, tie, _ = sample(img, lbl, draw, crop, dtype)
    if blur_k:
        p = blur(p, blur_k, dtype)
        p[~inside] = 0
    if jit:
        p[inside] = jitter(p[inside], alpha, beta, sigma, dtype)
    if lut is not None:
        lab = np.asarray(lut, dtype=np.int64)[lab]
    lab = np.where(inside, lab, ignore_label)
    out = []
    for m in (p, lab, ~inside, tie):
        if flip:
            m = np.flip(m, axis=1)
        out.append(np.rot90(m, k, (0, 1)))
    image, lab, pad, tie = out
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    if dtype == np.float64:
        image = (image[:, :, ::-1] / 255.0 - mean) / std
    else:
        image = (image[:, :, ::-1] / np.float32(255.0)).astype(np.float64) - mean
        image = (image.astype(np.float32).astype(np.float64) / std).astype(np.float32).astype(np.float64)
    return (np.ascontiguousarray(image.transpose(2, 0, 1)), (None if lbl is None else np.ascontiguousarray(lab)), np.ascontiguousarray(pad), np.ascontiguousarray(tie))


def source_rows_brute(img_shape, draw, crop):
    """(row0, rows) of the source rows the taps and labels of the inside pixels read, from the tap lists themselves; None when no pixel is inside."""
    H, W = img_shape
    rows = sample(np.zeros((H, W, 3), dtype=np.uint8), None, draw, crop)[4][0]
    if rows.size == 0:
        return None
    return int(rows.min()), int(rows.max() - rows.min() + 1)
