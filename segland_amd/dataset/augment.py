"""GPU tile preparation for the OpenEarthMap readers (counterpart of dataset/base_dataset.py:29-175 of the reference).

The reference prepares every tile on DataLoader worker CPUs (numpy + OpenCV); at >= 500 tiles/s per GPU that path starves the training step.
Here the workers only DECODE (rasterio) and hand over the raw uint8 tile; crop / pad / flip / rot90 / channel reversal / normalisation /
label re-indexing of a whole batch is one kernel launch (csrc/augment.hip).  The random draws are made on the host with the reference's
generators and in the reference's order, so a seeded run picks the same crops.

Two augmentations the reference does not have ride in the same launch when a reader is built with `augment=` (drivers: --aug-scale / --aug-jitter): a random rescale before the
crop (bilinear, labels nearest) and a brightness / contrast / saturation jitter.  Their draws are ExtDraw records, and a batch that holds one goes through sl_augment_batch_ex
(the contract: include/segland_hip.h); every other batch takes the path it always took."""
import collections
import ctypes as C
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


def draw_train_params(label, crop_size, ignore_label=255, mode='train', scale=None, jitter=None):
    """(h_off, w_off, flip, k): base_dataset.py:140-155 (np.random crop offsets, redrawn while the crop is all-ignore; outside train mode the
    crop is centred and nothing is drawn for it, :170-172), then :106-110 and :134-138 (one random.random() each for flip and rot90 count).

    scale=(lo, hi) and / or jitter=(b, c, s) (neither is in the reference; train mode only, any other mode draws what it drew and returns the 4-tuple): an ExtDraw, drawn in this
    order -- s = random.uniform(lo, hi) (only with scale=), Hs = max(1, int(H s + 0.5)) and Ws likewise; the crop offsets over (Hs, Ws), redrawn while the label window AS THE
    KERNEL SAMPLES IT (nearest, label_index) is all-ignore; flip and k; with jitter= alpha = 1 + U(-c, c), beta = U(-b, b), sigma = 1 + U(-s, s) from random.uniform.  With both
    off nothing else is drawn: seeded runs and the goldens G17 / G19 do not move."""
    H, W = label.shape
    ch, cw = crop_size
    if (scale is None and jitter is None) or mode != 'train':
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
    mh, mw = max(Hs - ch, 0), max(Ws - cw, 0)
    while True:
        h_off, w_off = np.random.randint(0, mh + 1), np.random.randint(0, mw + 1)
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
    return ExtDraw(int(h_off), int(w_off), flip, k, Hs, Ws, int(jitter is not None), alpha, beta, sigma, H, 0)


def augment_kwargs(augment):
    """The readers' `augment=` option -> the keyword arguments of draw_train_params: None, or a mapping with 'scale': (lo, hi) and / or 'jitter': (b, c, s) (absent or None: off)."""
    if not augment:
        return {}
    unknown = set(augment) - {'scale', 'jitter'}
    if unknown:
        raise ValueError("augment= takes 'scale' and 'jitter' (got %s)" % ', '.join(sorted(map(str, unknown))))
    kw = {}
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
    tensors, dataset/oem.py RawCollate); params: list of (h_off, w_off, flip, k) or ExtDraw."""

    def __init__(self, crop_size, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), ignore_label=255, lut=None, device='cuda'):
        self.crop_size, self.ignore_label, self.device = tuple(crop_size), ignore_label, torch.device(device)
        self.mean, self.std = (C.c_double * 3)(*mean), (C.c_double * 3)(*std)      # float64 like the python lists numpy broadcasts in normalize()
        self.lut = None if lut is None else torch.as_tensor(np.asarray(lut, dtype=np.uint8)).to(self.device)

    def prepare(self, tiles, params, order=None):
        """order: tile indices in output order (PairAugmenter: all novel tiles, then all base tiles); default 0..B-1."""
        ch, cw = self.crop_size
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

    def _record_ex(self, img_ptr, lbl_ptr, buf_rows, W, p):
        """The 80-byte record of include/segland_hip.h for one tile, with the checks the C side cannot make: the sizes, and that every source row the crop's taps read lies in
        the buffer (rows [row0, row0 + buf_rows) of the tile).  A plain draw is the identity rescale without jitter."""
        ch = self.crop_size[0]
        if len(p) > 4:
            h_off, w_off, flip, k, Hs, Ws, jitter, alpha, beta, sigma, H, row0 = p
        else:
            (h_off, w_off, flip, k), (Hs, Ws, jitter, alpha, beta, sigma, H, row0) = p, (buf_rows, W, 0, 1.0, 0.0, 1.0, buf_rows, 0)
        h_off, w_off, Hs, Ws, H, row0 = int(h_off), int(w_off), int(Hs), int(Ws), int(H), int(row0)
        if not (1 <= Hs <= MAX_SCALED and 1 <= Ws <= MAX_SCALED and 1 <= H <= MAX_TILE and 1 <= W <= MAX_TILE):
            raise ValueError('a %d x %d tile rescaled to %d x %d: tile sides must lie in [1, %d], rescaled sides in [1, %d]' % (H, W, Hs, Ws, MAX_TILE, MAX_SCALED))
        if h_off < 0 or w_off < 0 or buf_rows < 1 or row0 < 0 or row0 + buf_rows > H:
            raise ValueError('crop origin (%d, %d) / source rows [%d, %d) of a tile of %d rows: out of range' % (h_off, w_off, row0, row0 + buf_rows, H))
        if h_off < Hs and w_off < Ws:                   # else the whole crop is padding and nothing is read
            need0, need = source_rows(H, Hs, h_off, ch)
            if need0 < row0 or need0 + need > row0 + buf_rows:
                raise ValueError('the crop at row %d of the %d-row rescaled tile reads source rows [%d, %d); the buffer holds [%d, %d)'
                                 % (h_off, Hs, need0, need0 + need, row0, row0 + buf_rows))
        return struct.pack('<QQ11i3f2i', img_ptr, lbl_ptr, H, W, row0, buf_rows, Hs, Ws, h_off, w_off, int(bool(flip)), int(k) & 3, int(bool(jitter)),
                           float(alpha), float(beta) * 255.0, float(sigma), 0, 0)

    def _prepare_ex(self, tiles, params, order=None):
        """prepare() for a batch with extended draws (draw_train_params with scale= / jitter=): one sl_augment_batch_ex launch for the whole batch."""
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
                rec += self._record_ex(base + io, 0 if lo < 0 else base + lo, rows, W, p)
        else:
            with_label = tiles[order[0]][1] is not None
            for i, p in zip(order, params):
                img, lbl = tiles[i]
                if lbl is not None and tuple(lbl.shape) != tuple(img.shape[:2]):
                    raise ValueError('tile labels must be uint8 [H,W]')
                if len(p) > 4 and p.row0 == 0 and img.shape[0] == p.H and 0 <= p.h_off < p.Hs:
                    # only the rows the crop's taps read cross the bus (what crop_rows does in the workers)
                    row0, rows = source_rows(p.H, p.Hs, p.h_off, ch)
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
                rec += self._record_ex(it.data_ptr(), 0 if lt is None else lt.data_ptr(), it.shape[0], it.shape[1], p)
        table = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(self.device)
        out = torch.empty((B, 3, ch, cw), dtype=torch.float32, device=self.device)
        lab = torch.empty((B, ch, cw), dtype=torch.int64, device=self.device) if with_label else None
        _lib.check(_lib.lib().sl_augment_batch_ex(_p(table), B, ch, cw, self.mean, self.std, self.ignore_label, _p(self.lut), _p(out), _p(lab), _s()), 'augment_batch_ex')
        for t in keep:                                  # the raw tiles must outlive the kernel on this stream
            if t is not None:
                t.record_stream(torch.cuda.current_stream())
        return out, lab
