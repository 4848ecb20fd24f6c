"""GPU tile preparation for the OpenEarthMap readers (counterpart of dataset/base_dataset.py:29-175 of the reference).

The reference prepares every tile on DataLoader worker CPUs (numpy + OpenCV); at >= 500 tiles/s per GPU that path starves the training step.
Here the workers only DECODE (rasterio) and hand over the raw uint8 tile; crop / pad / flip / rot90 / channel reversal / normalisation /
label re-indexing of a whole batch is one kernel launch (csrc/augment.hip).  The random draws are made on the host with the reference's
generators and in the reference's order, so a seeded run picks the same crops.

Two augmentations the reference does not have ride in the same launch when a reader is built with `augment=` (drivers: --aug-scale / --aug-jitter): a random rescale before the
crop (bilinear, labels nearest) and a brightness / contrast / saturation jitter.  Their draws are ExtDraw records, and a batch that holds one goes through sl_augment_batch_ex
(the contract: include/segland_hip.h); every other batch takes the path it always took.

Two more are the reference's random_rotate and random_gaussian (base_dataset.py:112-132) under a contract of our own (--aug-rotate / --aug-blur): an arbitrary-angle rotation
about the crop centre and a separable Gaussian blur.  A draw in which one of them fired is a GeoDraw, and a batch that holds one goes through sl_augment_batch_geo."""
import collections
import ctypes as C
import math
import random
import struct

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _s

MAX_SCALED = 16384          # largest rescaled tile side of sl_augment_batch_ex: keeps (2Y + 1) H inside 32 bits
MAX_TILE = 32768


ExtDraw = collections.namedtuple('ExtDraw', 'h_off w_off flip k Hs Ws jitter alpha beta sigma H row0')
ExtDraw.__doc__ = """A draw with a rescale and / or a colour jitter (draw_train_params with scale= / jitter=).  h_off, w_off: crop origin in the RESCALED Hs x Ws grid; jitter 0 / 1 with
the factors alpha (contrast), beta (brightness, in units of the full range: the kernel gets float(beta * 255)) and sigma (saturation); H, row0: the full tile height and the
first source row of the buffer that travels with the draw (crop_rows cuts the tile down to the rows the crop reads and records where they start)."""


GeoDraw = collections.namedtuple('GeoDraw', ExtDraw._fields + ('rotate', 'cos_t', 'sin_t', 'blur_k'))
GeoDraw.__doc__ = """An ExtDraw with a rotation about the crop centre and / or a Gaussian blur (draw_train_params with rotate= / blur=): rotate 0 / 1 with the cosine and sine of
the angle (positive: counter-clockwise on the screen), blur_k 0 (off) or the odd kernel size 3..11."""

BLUR_SIZES = (3, 5, 7, 9, 11)


def blur_weights(K):
    """The six floats of the record: the half kernel of a K-tap Gaussian, centre first, sigma = 0.3 ((K - 1) / 2 - 1) + 0.8 (OpenCV's rule for sigma <= 0), computed in
    float64, normalised over the whole kernel, stored as float32; entries beyond the radius are 0."""
    if not K:
        return (0.0,) * 6
    R = (int(K) - 1) // 2
    sigma = 0.3 * ((K - 1) * 0.5 - 1.0) + 0.8
    g = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(R + 1)]
    total = g[0] + 2.0 * sum(g[1:])
    return tuple(g[i] / total if i <= R else 0.0 for i in range(6))


def geo_coords(ch, cw, h_off, w_off, cos_t, sin_t, rows=None, cols=None):
    """(U, V) float64 [len(rows), len(cols)]: step 2 of the contract of sl_augment_batch_geo for the crop positions rows x cols (default: the whole crop), with the kernel's
    order of operations."""
    r = np.arange(ch, dtype=np.float64) if rows is None else np.asarray(rows, dtype=np.float64)
    c = np.arange(cw, dtype=np.float64) if cols is None else np.asarray(cols, dtype=np.float64)
    hx, hy = 0.5 * cw, 0.5 * ch
    dx, dy = (c - hx)[None, :], (r - hy)[:, None]
    return w_off + (hx + (cos_t * dx - sin_t * dy)), h_off + (hy + (sin_t * dx + cos_t * dy))


def _nearest(P, S, Ss):
    """Step 4's label index of real rescaled coordinates P on an axis S -> Ss."""
    s = ((P + 0.5) * float(S)) / float(Ss) - 0.5
    return np.clip(np.floor(s + 0.5), 0, S - 1).astype(np.int64)


def rotated_label_window(label, Hs, Ws, h_off, w_off, ch, cw, cos_t, sin_t, step=1):
    """The labels the kernel reads for a rotated crop (steps 2-4 of the contract), 1-D, inside pixels only; step > 1 looks at every step-th row and column."""
    H, W = label.shape
    U, V = geo_coords(ch, cw, h_off, w_off, cos_t, sin_t, np.arange(0, ch, step), np.arange(0, cw, step))
    iu, iv = np.floor(U + 0.5), np.floor(V + 0.5)
    inside = (iu >= 0) & (iu < Ws) & (iv >= 0) & (iv < Hs)
    return label[_nearest(V[inside], H, Hs), _nearest(U[inside], W, Ws)]


def _check_rotation(cos_t, sin_t):
    if not (math.isfinite(cos_t) and math.isfinite(sin_t) and abs(math.hypot(cos_t, sin_t) - 1.0) < 1e-6):
        raise ValueError('rotation (cos %r, sin %r): not the cosine and sine of an angle' % (cos_t, sin_t))


def source_rows_geo(draw, ch, cw):
    """(row0, rows) covering every source row a tap or a label of the crop of `draw` can read.  Without a rotation: source_rows.  With one: V is linear in (r, c), so its
    extremes over the crop lie at the four corners; the interval (widened by 1e-6 against the last bit of the per-pixel evaluation, cut to the inside range [-0.5, Hs - 0.5])
    goes through step 4: from the upper tap of its low end to the lower tap of its high end, inside the tile.  The blur adds nothing: its taps stay inside the crop."""
    H, Hs = int(draw.H), int(draw.Hs)
    if not getattr(draw, 'rotate', 0):
        return source_rows(H, Hs, int(draw.h_off), ch)
    _check_rotation(draw.cos_t, draw.sin_t)
    _, V = geo_coords(ch, cw, draw.h_off, draw.w_off, draw.cos_t, draw.sin_t, (0, ch - 1), (0, cw - 1))
    sy = lambda v: ((min(max(v, -0.5), Hs - 0.5) + 0.5) * float(H)) / float(Hs) - 0.5      # noqa: E731
    lo, hi = sy(float(V.min()) - 1e-6), sy(float(V.max()) + 1e-6)
    row0 = int(math.floor(min(max(lo, 0.0), H - 1.0)))
    last = min(int(math.floor(min(max(hi, 0.0), H - 1.0))) + 1, H - 1)
    return row0, last - row0 + 1


def label_index(P, S, Ss):
    """Nearest source index of rescaled index P at the pixel centre: min(((2P + 1) S) // (2 Ss), S - 1) (step 4 of the contract in include/segland_hip.h)."""
    P = np.asarray(P, dtype=np.int64)
    return np.minimum(((2 * P + 1) * S) // (2 * Ss), S - 1)


def source_rows(H, Hs, h_off, ch):
    """(row0, rows): the source rows a crop of height ch at h_off of the rescaled tile reads -- from y0(h_off) to min(y0(Ymax) + 1, H - 1) with Ymax = min(h_off + ch, Hs) - 1,
    the upper and lower taps of its first and last row; the label rows (y0 or y0 + 1) lie within."""
    y0 = lambda Y: max((2 * Y + 1) * H - Hs, 0) // (2 * Hs)      # noqa: E731
    ymax = min(h_off + ch, Hs) - 1
    row0 = y0(h_off)
    return row0, min(y0(ymax) + 1, H - 1) - row0 + 1


def draw_train_params(label, crop_size, ignore_label=255, mode='train', scale=None, jitter=None, rotate=None, blur=None):
    """(h_off, w_off, flip, k): base_dataset.py:140-155 (np.random crop offsets, redrawn while the crop is all-ignore; outside train mode the
    crop is centred and nothing is drawn for it, :170-172), then :106-110 and :134-138 (one random.random() each for flip and rot90 count).

    scale=(lo, hi) and / or jitter=(b, c, s) (neither is in the reference; train mode only, any other mode draws what it drew and returns the 4-tuple): an ExtDraw, drawn in this
    order -- s = random.uniform(lo, hi) (only with scale=), Hs = max(1, int(H s + 0.5)) and Ws likewise; the crop offsets over (Hs, Ws), redrawn while the label window AS THE
    KERNEL SAMPLES IT (nearest, label_index) is all-ignore; flip and k; with jitter= alpha = 1 + U(-c, c), beta = U(-b, b), sigma = 1 + U(-s, s) from random.uniform.  With both
    off nothing else is drawn: seeded runs and the goldens G17 / G19 do not move.

    rotate=(lo, hi, p) and / or blur=(K, p) (train mode only; the reference's random_rotate / random_gaussian under the contract of sl_augment_batch_geo): the order becomes --
    the scale draw; with rotate= random.random() < p and, if that holds, angle = lo + (hi - lo) random.random() in degrees; the crop offsets, redrawn while the label window as
    the kernel samples it THROUGH THE ROTATION is all-ignore (a coarse sub-grid of that window may accept a draw early; the full window decides otherwise); flip, k and the
    jitter; with blur= random.random() < p.  A draw in which neither fired is returned as without the two options (an ExtDraw, or the 4-tuple when scale and jitter are off
    too); otherwise a GeoDraw."""
    H, W = label.shape
    ch, cw = crop_size
    if (scale is None and jitter is None and rotate is None and blur is None) or mode != 'train':
        mh, mw = max(H - ch, 0), max(W - cw, 0)
        if mode == 'train':
            while True:
                h_off, w_off = np.random.randint(0, mh + 1), np.random.randint(0, mw + 1)
                u = np.unique(label[h_off:h_off + ch, w_off:w_off + cw])
                if not (u.size == 1 and int(u[0]) == ignore_label):
                    break
        else:
            h_off, w_off = int(round(mh / 2.)), int(round(mw / 2.))
        flip = random.random() < 0.5
        k = int(random.random() // 0.25)
        return h_off, w_off, flip, k
    Hs, Ws = H, W
    if scale is not None:
        s = random.uniform(scale[0], scale[1])
        Hs, Ws = max(1, int(H * s + 0.5)), max(1, int(W * s + 0.5))
    if not (1 <= Hs <= MAX_SCALED and 1 <= Ws <= MAX_SCALED):
        raise ValueError('a %d x %d tile rescaled to %d x %d: the rescaled size must lie in [1, %d]' % (H, W, Hs, Ws, MAX_SCALED))
    rot, cos_t, sin_t = 0, 1.0, 0.0
    if rotate is not None and random.random() < rotate[2]:
        angle = rotate[0] + (rotate[1] - rotate[0]) * random.random()
        rot, cos_t, sin_t = 1, math.cos(math.radians(angle)), math.sin(math.radians(angle))
    mh, mw = max(Hs - ch, 0), max(Ws - cw, 0)
    while True:
        h_off, w_off = np.random.randint(0, mh + 1), np.random.randint(0, mw + 1)
        if rot:
            if (rotated_label_window(label, Hs, Ws, h_off, w_off, ch, cw, cos_t, sin_t, 16) != ignore_label).any():
                break
            u = np.unique(rotated_label_window(label, Hs, Ws, h_off, w_off, ch, cw, cos_t, sin_t))
        else:
            rows = label_index(np.arange(h_off, min(h_off + ch, Hs)), H, Hs)
            cols = label_index(np.arange(w_off, min(w_off + cw, Ws)), W, Ws)
            u = np.unique(label[rows][:, cols])
        if not (u.size == 1 and int(u[0]) == ignore_label):
            break
    flip = random.random() < 0.5
    k = int(random.random() // 0.25)
    alpha, beta, sigma = 1.0, 0.0, 1.0
    if jitter is not None:
        b, c, sat = jitter
        alpha = 1.0 + random.uniform(-c, c)
        beta = random.uniform(-b, b)
        sigma = 1.0 + random.uniform(-sat, sat)
    blur_k = int(blur[0]) if blur is not None and random.random() < blur[1] else 0
    if rot or blur_k:
        return GeoDraw(int(h_off), int(w_off), flip, k, Hs, Ws, int(jitter is not None), alpha, beta, sigma, H, 0, rot, cos_t, sin_t, blur_k)
    if scale is None and jitter is None:
        return int(h_off), int(w_off), flip, k
    return ExtDraw(int(h_off), int(w_off), flip, k, Hs, Ws, int(jitter is not None), alpha, beta, sigma, H, 0)


def augment_kwargs(augment, crop_size=None):
    """The readers' `augment=` option -> the keyword arguments of draw_train_params: None, or a mapping with 'scale': (lo, hi), 'jitter': (b, c, s), 'rotate': (lo, hi[, p]) in
    degrees and / or 'blur': (K[, p]) (absent or None: off; p defaults to 0.5 as in the reference).  crop_size: the reader's crop, whose sides a blur radius must stay below."""
    if not augment:
        return {}
    unknown = set(augment) - {'scale', 'jitter', 'rotate', 'blur'}
    if unknown:
        raise ValueError("augment= takes 'scale', 'jitter', 'rotate' and 'blur' (got %s)" % ', '.join(sorted(map(str, unknown))))
    kw = {}
    if augment.get('rotate'):
        r = tuple(map(float, augment['rotate']))
        if len(r) not in (2, 3) or not -180.0 <= r[0] <= r[1] <= 180.0:
            raise ValueError('augment rotate range must satisfy -180 <= lo <= hi <= 180 (got %r)' % (augment['rotate'],))
        p = r[2] if len(r) == 3 else 0.5
        if not 0.0 < p <= 1.0:
            raise ValueError('augment rotate probability must lie in (0, 1] (got %r)' % (augment['rotate'],))
        kw['rotate'] = (r[0], r[1], p)
    if augment.get('blur'):
        bl = tuple(map(float, augment['blur']))
        if len(bl) not in (1, 2) or bl[0] not in BLUR_SIZES:
            raise ValueError('augment blur size must be one of %s (got %r)' % (', '.join(map(str, BLUR_SIZES)), augment['blur']))
        p = bl[1] if len(bl) == 2 else 0.5
        if not 0.0 < p <= 1.0:
            raise ValueError('augment blur probability must lie in (0, 1] (got %r)' % (augment['blur'],))
        if crop_size is not None and min(crop_size) <= (int(bl[0]) - 1) // 2:
            raise ValueError('a %d-tap blur needs crop sides above %d (got %r)' % (int(bl[0]), (int(bl[0]) - 1) // 2, tuple(crop_size)))
        kw['blur'] = (int(bl[0]), p)
    if augment.get('scale'):
        lo, hi = map(float, augment['scale'])
        if not 0.0 < lo <= hi:
            raise ValueError('augment scale range must satisfy 0 < lo <= hi (got %r)' % (augment['scale'],))
        kw['scale'] = (lo, hi)
    if augment.get('jitter'):
        b, c, s = map(float, augment['jitter'])
        if not all(0.0 <= v < 1.0 for v in (b, c, s)):
            raise ValueError('augment jitter amplitudes must lie in [0, 1) (got %r)' % (augment['jitter'],))
        kw['jitter'] = (b, c, s)
    return kw


def remap_lut(base_classes, novel_classes, use_base=True, use_novel=True):
    """dataset/oem.py:113-133 as a lookup table (uint8[256])."""
    lut = np.arange(256, dtype=np.uint8)
    base, novel = list(base_classes), list(novel_classes)
    for c in base:
        lut[c] = base.index(c) + 1 if use_base else 0
    for c in novel:
        lut[c] = (novel.index(c) + (len(base) + 1 if use_base else 1)) if use_novel else 0
    return lut


class TileAugmenter:
    """prepare(tiles, params) -> (image [B,3,ch,cw] float32, label [B,ch,cw] int64) on the GPU.
    tiles: list of (image uint8 [H,W,3], label uint8 [H,W] or None) numpy arrays or CPU tensors (what the readers' collate functions hand over: shared-memory
    tensors, dataset/oem.py RawCollate); params: list of (h_off, w_off, flip, k), ExtDraw or GeoDraw."""

    def __init__(self, crop_size, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), ignore_label=255, lut=None, device='cuda'):
        self.crop_size, self.ignore_label, self.device = tuple(crop_size), ignore_label, torch.device(device)
        self.mean, self.std = (C.c_double * 3)(*mean), (C.c_double * 3)(*std)      # float64 like the python lists numpy broadcasts in normalize()
        self.lut = None if lut is None else torch.as_tensor(np.asarray(lut, dtype=np.uint8)).to(self.device)

    def prepare(self, tiles, params, order=None):
        """order: tile indices in output order (PairAugmenter: all novel tiles, then all base tiles); default 0..B-1."""
        ch, cw = self.crop_size
        if any(isinstance(p, GeoDraw) for p in params):   # a rotation or a blur somewhere in the batch: the whole batch goes through sl_augment_batch_geo
            return self._prepare_ex(tiles, params, order, geo=True)
        if any(len(p) > 4 for p in params):               # a rescale or a jitter somewhere in the batch: the whole batch goes through sl_augment_batch_ex
            return self._prepare_ex(tiles, params, order)
        if any(k % 2 for _, _, _, k in params) and ch != cw:
            raise ValueError('rot90 by an odd count needs square crops')
        from .oem import PackedTiles
        B = len(params)
        order = list(range(B)) if order is None else list(order)
        keep, rec, flags = [], b'', []
        if isinstance(tiles, PackedTiles):
            # one host -> device copy for the whole batch (the collate in the worker packed it, already cut down to the crops' rows)
            dbuf = tiles.buf.to(self.device, non_blocking=True)
            base = dbuf.data_ptr()
            keep.append(dbuf)
            with_label = tiles.meta[order[0]][3] >= 0
            for i, (h_off, w_off, flip, k) in zip(order, params):
                io, H, W, lo = tiles.meta[i]
                rec += struct.pack('<QQiiii', base + io, 0 if lo < 0 else base + lo, H, W, int(h_off), int(w_off))
                flags += [int(bool(flip)), int(k) & 3]
        else:
            with_label = tiles[order[0]][1] is not None
            for i, (h_off, w_off, flip, k) in zip(order, params):
                img, lbl = tiles[i]
                if lbl is not None and tuple(lbl.shape) != tuple(img.shape[:2]):
                    raise ValueError('tile labels must be uint8 [H,W]')
                # only the rows the crop reads cross the bus: a tile at least as tall as the crop is never padded vertically (base_dataset.py:88-104 pads a tile
                # that is SMALLER than the crop), so rows [h_off, h_off + ch) -- a contiguous slice of the row-major tile -- are all the kernel looks at (1.5 instead
                # of 3 MB for a 512-row crop of a 1024 x 1024 RGB tile)
                if img.shape[0] > ch and 0 <= h_off <= img.shape[0] - ch:
                    img = img[h_off:h_off + ch]
                    lbl = None if lbl is None else lbl[h_off:h_off + ch]
                    h_off = 0
                it = (img.contiguous() if isinstance(img, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(img))).to(self.device, non_blocking=True)
                if it.dtype != torch.uint8 or it.dim() != 3 or it.shape[2] != 3:
                    raise ValueError('tile images must be uint8 [H,W,3]')
                lt = None
                if lbl is not None:
                    lt = (lbl.contiguous() if isinstance(lbl, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(lbl))).to(self.device, non_blocking=True)
                    if lt.dtype != torch.uint8 or tuple(lt.shape) != tuple(it.shape[:2]):
                        raise ValueError('tile labels must be uint8 [H,W]')
                keep += [it, lt]
                rec += struct.pack('<QQiiii', it.data_ptr(), 0 if lt is None else lt.data_ptr(), it.shape[0], it.shape[1], int(h_off), int(w_off))
                flags += [int(bool(flip)), int(k) & 3]
        table = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(self.device)
        fl = torch.tensor(flags, dtype=torch.int32).to(self.device)
        out = torch.empty((B, 3, ch, cw), dtype=torch.float32, device=self.device)
        lab = torch.empty((B, ch, cw), dtype=torch.int64, device=self.device) if with_label else None
        _lib.check(_lib.lib().sl_augment_batch(_p(table), _p(fl), B, ch, cw, self.mean, self.std, self.ignore_label, _p(self.lut), _p(out), _p(lab), _s()), 'augment_batch')
        for t in keep:                                  # the raw tiles must outlive the kernel on this stream
            if t is not None:
                t.record_stream(torch.cuda.current_stream())
        return out, lab

    def _record_ex(self, img_ptr, lbl_ptr, buf_rows, W, p, geo=False):
        """The 80-byte record of include/segland_hip.h for one tile (geo: the 128-byte one of sl_augment_batch_geo), with the checks the C side cannot make: the sizes, and that
        every source row the crop's taps read lies in the buffer (rows [row0, row0 + buf_rows) of the tile).  A plain draw is the identity rescale without jitter, and in a geo
        batch every draw that is no GeoDraw has rotate = blur_k = 0."""
        ch, cw = self.crop_size
        rotate, cos_t, sin_t, blur_k = p[12:16] if isinstance(p, GeoDraw) else (0, 1.0, 0.0, 0)
        if len(p) > 4:
            h_off, w_off, flip, k, Hs, Ws, jitter, alpha, beta, sigma, H, row0 = p[:12]
        else:
            (h_off, w_off, flip, k), (Hs, Ws, jitter, alpha, beta, sigma, H, row0) = p, (buf_rows, W, 0, 1.0, 0.0, 1.0, buf_rows, 0)
        h_off, w_off, Hs, Ws, H, row0 = int(h_off), int(w_off), int(Hs), int(Ws), int(H), int(row0)
        if not (1 <= Hs <= MAX_SCALED and 1 <= Ws <= MAX_SCALED and 1 <= H <= MAX_TILE and 1 <= W <= MAX_TILE):
            raise ValueError('a %d x %d tile rescaled to %d x %d: tile sides must lie in [1, %d], rescaled sides in [1, %d]' % (H, W, Hs, Ws, MAX_TILE, MAX_SCALED))
        if h_off < 0 or w_off < 0 or buf_rows < 1 or row0 < 0 or row0 + buf_rows > H:
            raise ValueError('crop origin (%d, %d) / source rows [%d, %d) of a tile of %d rows: out of range' % (h_off, w_off, row0, row0 + buf_rows, H))
        if blur_k and (int(blur_k) not in BLUR_SIZES or min(ch, cw) <= (int(blur_k) - 1) // 2):
            raise ValueError('blur size %r on a %d x %d crop: the size must be one of %s and the crop sides above its radius' % (blur_k, ch, cw, ', '.join(map(str, BLUR_SIZES))))
        if rotate:
            _check_rotation(cos_t, sin_t)
        if rotate or (h_off < Hs and w_off < Ws):       # else the whole crop is padding and nothing is read
            need0, need = source_rows_geo(p, ch, cw) if rotate else source_rows(H, Hs, h_off, ch)
            if need0 < row0 or need0 + need > row0 + buf_rows:
                raise ValueError('the crop at row %d of the %d-row rescaled tile reads source rows [%d, %d); the buffer holds [%d, %d)'
                                 % (h_off, Hs, need0, need0 + need, row0, row0 + buf_rows))
        head = struct.pack('<QQ11i3f', img_ptr, lbl_ptr, H, W, row0, buf_rows, Hs, Ws, h_off, w_off, int(bool(flip)), int(k) & 3, int(bool(jitter)),
                           float(alpha), float(beta) * 255.0, float(sigma))
        if not geo:
            return head + struct.pack('<2i', 0, 0)
        return head + struct.pack('<2i2d6f2i', int(bool(rotate)), int(blur_k), float(cos_t), float(sin_t), *blur_weights(int(blur_k)), 0, 0)

    def _prepare_ex(self, tiles, params, order=None, geo=False):
        """prepare() for a batch with extended draws (draw_train_params with scale= / jitter=): one sl_augment_batch_ex launch for the whole batch; geo: a batch that holds a
        GeoDraw (rotate= / blur=), one sl_augment_batch_geo launch."""
        ch, cw = self.crop_size
        if any(p[3] % 2 for p in params) and ch != cw:
            raise ValueError('rot90 by an odd count needs square crops')
        from .oem import PackedTiles
        B = len(params)
        order = list(range(B)) if order is None else list(order)
        keep, rec = [], b''
        if isinstance(tiles, PackedTiles):
            dbuf = tiles.buf.to(self.device, non_blocking=True)
            base = dbuf.data_ptr()
            keep.append(dbuf)
            with_label = tiles.meta[order[0]][3] >= 0
            for i, p in zip(order, params):
                io, rows, W, lo = tiles.meta[i]
                rec += self._record_ex(base + io, 0 if lo < 0 else base + lo, rows, W, p, geo)
        else:
            with_label = tiles[order[0]][1] is not None
            for i, p in zip(order, params):
                img, lbl = tiles[i]
                if lbl is not None and tuple(lbl.shape) != tuple(img.shape[:2]):
                    raise ValueError('tile labels must be uint8 [H,W]')
                if len(p) > 4 and p.row0 == 0 and img.shape[0] == p.H and (getattr(p, 'rotate', 0) or 0 <= p.h_off < p.Hs):
                    # only the rows the crop's taps read cross the bus (what crop_rows does in the workers)
                    row0, rows = source_rows_geo(p, ch, cw)
                    img, lbl, p = img[row0:row0 + rows], (None if lbl is None else lbl[row0:row0 + rows]), p._replace(row0=row0)
                it = (img.contiguous() if isinstance(img, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(img))).to(self.device, non_blocking=True)
                if it.dtype != torch.uint8 or it.dim() != 3 or it.shape[2] != 3:
                    raise ValueError('tile images must be uint8 [H,W,3]')
                lt = None
                if lbl is not None:
                    lt = (lbl.contiguous() if isinstance(lbl, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(lbl))).to(self.device, non_blocking=True)
                    if lt.dtype != torch.uint8 or tuple(lt.shape) != tuple(it.shape[:2]):
                        raise ValueError('tile labels must be uint8 [H,W]')
                keep += [it, lt]
                rec += self._record_ex(it.data_ptr(), 0 if lt is None else lt.data_ptr(), it.shape[0], it.shape[1], p, geo)
        table = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(self.device)
        out = torch.empty((B, 3, ch, cw), dtype=torch.float32, device=self.device)
        lab = torch.empty((B, ch, cw), dtype=torch.int64, device=self.device) if with_label else None
        if geo:
            _lib.check(_lib.lib().sl_augment_batch_geo(_p(table), B, ch, cw, self.mean, self.std, self.ignore_label, _p(self.lut), _p(out), _p(lab), _s()), 'augment_batch_geo')
        else:
            _lib.check(_lib.lib().sl_augment_batch_ex(_p(table), B, ch, cw, self.mean, self.std, self.ignore_label, _p(self.lut), _p(out), _p(lab), _s()), 'augment_batch_ex')
        for t in keep:                                  # the raw tiles must outlive the kernel on this stream
            if t is not None:
                t.record_stream(torch.cuda.current_stream())
        return out, lab
