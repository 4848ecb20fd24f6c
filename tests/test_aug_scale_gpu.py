"""sl_augment_batch_ex on the GPU: random rescale before the crop and colour jitter behind it, in the one launch that prepares a batch (csrc/augment.hip; the contract is the
comment in include/segland_hip.h, restated in float64 by aug_reference.py).  With the identity rescale and no jitter the new entry is sl_augment_batch bit for bit; with them
labels and padding are exact and the image holds atol 2e-5 on the normalised values: the float32 chain has about 20 roundings on magnitudes <= 510 behind factors <= 2, below
4e-5 in the worst case; a float32 numpy evaluation of the reference on these shapes and factors stays at 1.3e-6, so 2e-5 leaves a 15x margin for summation order and nothing
more.  Tiles <= 64 x 64, crops 32 x 32."""
import glob
import logging
import os
import random
import re

import numpy as np
import pytest
import torch

import aug_reference as ar

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CH = CW = 32
MEAN = STD = (0.5, 0.5, 0.5)
ATOL = 2e-5
SIZES = [(40, 56), (37, 53), (64, 64)]
SCALES = [0.5, 0.73, 1.37, 2.0, 3.99]
TRIPLES = [None, (1.4, 0.2, 1.5), (0.6, -0.2, 0.5), (1.99, 0.5, 1.99)]        # (alpha, beta, sigma); None: jitter off
LUT = ((np.arange(256) * 7 + 3) % 251).astype(np.uint8)


def _tiles(seed=0, sizes=SIZES, ignore_rows=3):
    rng = np.random.RandomState(seed)
    out = []
    for h, w in sizes:
        lab = rng.randint(0, 12, (h, w)).astype(np.uint8)
        lab[:ignore_rows] = 255
        out.append((rng.randint(0, 256, (h, w, 3)).astype(np.uint8), lab))
    return out


def _ext(h_off, w_off, flip, k, Hs, Ws, triple, H):
    from segland_amd.dataset.augment import ExtDraw
    a, b, s = triple or (1.0, 0.0, 1.0)
    return ExtDraw(h_off, w_off, flip, k, Hs, Ws, int(triple is not None), a, b, s, H, 0)


def _augmenter(lut=None, mean=MEAN, std=STD):
    from segland_amd.dataset.augment import TileAugmenter
    return TileAugmenter((CH, CW), mean, std, 255, lut=lut, device=DEV)


# --------------------------------------------------------------------------------------------- identity rescale, no jitter: the old entry bit for bit
@pytest.mark.parametrize('lut', [None, LUT], ids=['nolut', 'lut'])
def test_identity_rescale_equals_the_plain_entry_bit_for_bit(hip, lut):
    """Every flip x k, tiles larger than the crop at several offsets and one SMALLER than it (padded on two sides), with and without the label table."""
    tiles = _tiles(1, SIZES + [(20, 28)])
    aug = _augmenter(lut)
    plain, ext, batch = [], [], []
    for flip in (False, True):
        for k in range(4):
            for t, (img, lab) in enumerate(tiles):
                H, W = lab.shape
                mh, mw = max(H - CH, 0), max(W - CW, 0)
                for h_off, w_off in {(0, 0), (mh, mw), (mh // 2, mw // 3)}:
                    batch.append((img, lab))
                    plain.append((h_off, w_off, flip, k))
                    ext.append(_ext(h_off, w_off, flip, k, H, W, None, H))
    want_i, want_l = aug.prepare(batch, plain)
    got_i, got_l = aug.prepare(batch, ext)
    assert torch.equal(got_i, want_i) and torch.equal(got_l, want_l)
    # a batch that mixes plain and extended draws goes through the new entry as a whole: the plain ones are the identity rescale
    mixed = [e if i % 2 else p for i, (p, e) in enumerate(zip(plain, ext))]
    mix_i, mix_l = aug.prepare(batch, mixed)
    assert torch.equal(mix_i, want_i) and torch.equal(mix_l, want_l)
    assert (want_l == 255).any() and len(batch) >= 8 * 4


def test_identity_rescale_of_unlabeled_tiles(hip):
    tiles = [(img, None) for img, _ in _tiles(2, SIZES + [(20, 28)])]
    aug = _augmenter()
    plain = [(i % 3, (2 * i) % 5, bool(i % 2), i % 4) for i in range(len(tiles))]
    ext = [_ext(p[0], p[1], p[2], p[3], t[0].shape[0], t[0].shape[1], None, t[0].shape[0]) for p, t in zip(plain, tiles)]
    want_i, want_l = aug.prepare(tiles, plain)
    got_i, got_l = aug.prepare(tiles, ext)
    assert want_l is None and got_l is None and torch.equal(got_i, want_i)


# --------------------------------------------------------------------------------------------- parity with the float64 reference
_RESAMPLED = {}


def _resampled(t, img, Hs, Ws):
    key = (t, Hs, Ws)
    if key not in _RESAMPLED:
        _RESAMPLED[key] = ar.resample(img, Hs, Ws)
    return _RESAMPLED[key]


@pytest.mark.parametrize('triple', TRIPLES, ids=['nojitter', 'strong', 'weak', 'strongest'])
def test_rescale_and_jitter_match_the_float64_reference(hip, triple):
    """3 tiles of different sizes x 5 scale assignments (every tile meets every scale; at 0.5 the rescaled 20 x 28 tile is smaller than the crop) x flip x k x offsets at 0 and
    at the far edge, one launch per scale assignment.  Labels and padding exact, image within ATOL."""
    tiles = _tiles(3)
    aug = _augmenter(LUT)
    worst, npad = 0.0, 0
    for rot in range(len(SCALES)):
        batch, draws, which = [], [], []
        for t, (img, lab) in enumerate(tiles):
            H, W = lab.shape
            s = SCALES[(rot + t) % len(SCALES)]
            Hs, Ws = ar.scaled_size(H, s), ar.scaled_size(W, s)
            for flip in (False, True):
                for k in range(4):
                    for h_off, w_off in ((0, 0), (max(Hs - CH, 0), max(Ws - CW, 0))):
                        batch.append((img, lab))
                        draws.append(_ext(h_off, w_off, flip, k, Hs, Ws, triple, H))
                        which.append(t)
        got_i, got_l = aug.prepare(batch, draws)
        got_i, got_l = got_i.cpu().numpy().astype(np.float64), got_l.cpu().numpy()
        for j, (d, t) in enumerate(zip(draws, which)):
            img, lab = tiles[t]
            want_i, want_l, pad = ar.prepare(img, lab, d, (CH, CW), MEAN, STD, 255, LUT, resampled=_resampled(t, img, d.Hs, d.Ws))
            assert np.array_equal(got_l[j], want_l), (rot, j, d)
            assert np.array_equal(got_l[j][pad], np.full(int(pad.sum()), 255))
            assert np.array_equal(got_i[j][:, pad], np.broadcast_to(((0.0 - np.array(MEAN)) / np.array(STD))[:, None], (3, int(pad.sum())))), (rot, j, d)      # 0 before normalisation, exactly
            worst = max(worst, float(np.abs(got_i[j] - want_i).max()))
            npad += int(pad.sum())
    print('rescale + jitter %s: max |kernel - float64 reference| on the normalised image %.3g (bound %.0e), %d padding pixels' % (triple, worst, ATOL, npad))
    assert npad > 0
    assert worst <= ATOL


def test_clip_saturation(hip):
    """All-255 and all-0 tiles under the strongest triple, and its mirror image: every clip of the jitter stage is hit from both sides."""
    aug = _augmenter()
    worst = 0.0
    for triple in ((1.99, 0.5, 1.99), (1.99, -0.5, 1.99), (0.01, 0.5, 0.01)):
        batch, draws = [], []
        for value in (255, 0):
            img = np.full((40, 56, 3), value, dtype=np.uint8)
            img[:, :, 1] = value if value else 0
            lab = np.zeros((40, 56), dtype=np.uint8)
            batch.append((img, lab))
            draws.append(_ext(5, 7, False, 0, 55, 77, triple, 40))
        mixed = np.zeros((40, 56, 3), dtype=np.uint8)
        mixed[:, :, 0] = 255                                  # a saturated colour: the saturation stage pushes channels past both ends
        batch.append((mixed, np.zeros((40, 56), dtype=np.uint8)))
        draws.append(_ext(5, 7, True, 2, 55, 77, triple, 40))
        got = aug.prepare(batch, draws)[0].cpu().numpy().astype(np.float64)
        for j in range(3):
            want = ar.prepare(batch[j][0], batch[j][1], draws[j], (CH, CW), MEAN, STD)[0]
            worst = max(worst, float(np.abs(got[j] - want).max()))
            assert want.min() >= -1.0 and want.max() <= 1.0
    print('clip saturation: max |kernel - float64 reference| %.3g' % worst)
    assert worst <= ATOL


def test_two_runs_give_the_same_bits(hip):
    tiles = _tiles(4)
    aug = _augmenter()
    draws = [_ext(3, 4, bool(t % 2), t, ar.scaled_size(l.shape[0], 1.37), ar.scaled_size(l.shape[1], 1.37), (1.4, 0.2, 1.5), l.shape[0]) for t, (_, l) in enumerate(tiles)]
    a, b = aug.prepare(tiles, draws), aug.prepare(tiles, draws)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# --------------------------------------------------------------------------------------------- what the Python side refuses, and the C side before any launch
def test_bad_sizes_and_buffers_are_refused(hip):
    from segland_amd import _lib
    from segland_amd.ops import _p, _s
    tiles = _tiles(5)[:1]
    aug = _augmenter()
    H, W = tiles[0][1].shape
    with pytest.raises(ValueError, match='rescaled'):
        aug.prepare(tiles, [_ext(0, 0, False, 0, 16385, W, None, H)])
    with pytest.raises(ValueError, match='rescaled'):
        aug.prepare(tiles, [_ext(0, 0, False, 0, H, 0, None, H)])
    with pytest.raises(ValueError, match='reads source rows'):      # a buffer that does not hold the rows the crop's taps need
        aug.prepare([(tiles[0][0][:10], tiles[0][1][:10])], [_ext(0, 0, False, 0, H, W, None, H)._replace(row0=0)])
    with pytest.raises(ValueError, match='out of range'):
        aug.prepare(tiles, [_ext(-1, 0, False, 0, H, W, None, H)])
    with pytest.raises(ValueError, match='square'):
        from segland_amd.dataset.augment import TileAugmenter
        TileAugmenter((32, 16), MEAN, STD, 255, device=DEV).prepare(tiles, [_ext(0, 0, False, 1, H, W, None, H)])
    lib = _lib.lib()
    out = torch.empty((1, 3, CH, CW), device=DEV)
    table = torch.zeros(80, dtype=torch.uint8, device=DEV)
    for args in ((None, 1, CH, CW, aug.mean, aug.std, _p(out)), (_p(table), 0, CH, CW, aug.mean, aug.std, _p(out)), (_p(table), 1, 0, CW, aug.mean, aug.std, _p(out)),
                 (_p(table), 1, CH, -1, aug.mean, aug.std, _p(out)), (_p(table), 1, CH, CW, None, aug.std, _p(out)), (_p(table), 1, CH, CW, aug.mean, None, _p(out)),
                 (_p(table), 1, CH, CW, aug.mean, aug.std, None)):
        t, B, ch, cw, m, s, o = args
        assert lib.sl_augment_batch_ex(t, B, ch, cw, m, s, 255, None, o, None, _s()) != 0


# --------------------------------------------------------------------------------------------- row slicing in the workers' collate
def test_row_sliced_packed_tiles_prepare_identically(hip):
    """The same batch as a list of whole arrays, packed whole (RawCollate(None)) and packed after the collate cut every tile down to the rows its crop's taps read."""
    from segland_amd.dataset.oem import PackedTiles, RawCollate
    tiles = _tiles(6)
    aug = _augmenter()
    draws, batch = [], []
    for rot in range(len(SCALES)):
        for t, (img, lab) in enumerate(tiles):
            H, W = lab.shape
            s = SCALES[(rot + t) % len(SCALES)]
            Hs, Ws = ar.scaled_size(H, s), ar.scaled_size(W, s)
            for edge in (0, 1, 2):
                h_off, w_off = (0, 0) if edge == 0 else (max(Hs - CH, 0) // (3 - edge), max(Ws - CW, 0) // (3 - edge))
                draws.append(_ext(h_off, w_off, bool(edge % 2), (rot + edge) % 4, Hs, Ws, TRIPLES[(rot + edge) % 4], H))
                batch.append((img, lab))
    draws.append((2, 3, True, 3))                             # a plain draw among them
    batch.append(tiles[2])
    want_i, want_l = aug.prepare(batch, draws)
    samples = [(b[0], b[1], d, i) for i, (b, d) in enumerate(zip(batch, draws))]
    whole, pw, _ = RawCollate(None)(samples)
    cut, pc, _ = RawCollate(CH)(samples)
    assert isinstance(cut, PackedTiles) and cut.buf.numel() < whole.buf.numel()
    assert any(p.row0 > 0 for p in pc[:-1]) and all(cut[i][0].shape[0] <= batch[i][0].shape[0] for i in range(len(batch)))
    for packed, prm in ((whole, pw), (cut, pc)):
        got_i, got_l = aug.prepare(packed, prm)
        assert torch.equal(got_i, want_i) and torch.equal(got_l, want_l)


# --------------------------------------------------------------------------------------------- pairs
def test_pair_augmenter_with_the_options_equals_the_reference_per_tile(hip):
    from segland_amd.dataset import oem_ft, synthetic_raw_ft
    random.seed(11)
    np.random.seed(11)
    ds = synthetic_raw_ft.GFSSegTrain(crop_size=(CH, CW), shot=2, length=12, tile=(60, 64), augment={'scale': (0.5, 2.0), 'jitter': (0.3, 0.3, 0.3)})
    samples = [ds[0], ds[5]]
    packed, params, _ = ds.collate_fn(samples)
    img, mask, img_b, mask_b = ds.augmenter(DEV).prepare(packed, params)
    assert img.shape == (2, 3, CH, CW) and mask_b.dtype == torch.int64
    worst = 0.0
    for i, ((nov, base), (pn, pb), _) in enumerate(samples):
        assert len(pn) > 4 and len(pb) > 4 and pn != pb
        for (tile, d, gi, gl) in ((nov, pn, img[i], mask[i]), (base, pb, img_b[i], mask_b[i])):
            want_i, want_l, _ = ar.prepare(tile[0], tile[1], d, (CH, CW), oem_ft.MEAN, oem_ft.STD, 255)
            assert np.array_equal(gl.cpu().numpy(), want_l)
            worst = max(worst, float(np.abs(gi.cpu().numpy().astype(np.float64) - want_i).max()))
    print('pairs: max |kernel - float64 reference| on the normalised image (ImageNet statistics) %.3g' % worst)
    assert worst <= ATOL


# --------------------------------------------------------------------------------------------- drivers
def _count_calls(monkeypatch):
    from segland_amd import _lib
    lib = _lib.lib()
    calls = {'sl_augment_batch': 0, 'sl_augment_batch_ex': 0}
    for name in calls:
        fn = getattr(lib, name)

        def wrapper(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapper)
    return calls


@pytest.mark.parametrize('ft', [False, True], ids=['train_base', 'ft_pop'])
def test_drivers_train_with_the_augmentation_flags(hip, tmp_path, caplog, monkeypatch, ft):
    """One short epoch on synthetic_raw (the readers' raw-tile format without a decode) with both flags: finite losses and weights, the start-up line, every training batch
    through the new entry; the same run without the flags never reaches it."""
    from segland_amd import ft_pop, train_base
    calls = _count_calls(monkeypatch)
    common = ['--model', 'pspnet_pop', '--backbone', 'resnet50', '--dataset', 'synthetic_raw', '--input-size', '128,128', '--base-size', '128,128', '--num-epoch', '1',
              '--restore-from', '/nonexistent', '--allow-random-init']
    common += (['--batch-size', '4', '--learning-rate', '1e-3', '--print-frequency', '1', '--random-seed', '123', '--freeze-backbone', '--fix-bn', '--shot', '2'] if ft
               else ['--batch-size', '4', '--learning-rate', '1e-4', '--print-frequency', '4', '--fp16'])
    main = ft_pop.main if ft else train_base.main
    snap = str(tmp_path / 'on')
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        main(common + ['--snapshot-dir', snap, '--num-workers', '2', '--aug-scale', '0.5,2.0', '--aug-jitter', '0.2,0.2,0.2'])
    text = '\n'.join(r.getMessage() for r in caplog.records)
    assert 'random rescale 0.5..2 before the crop' in text and 'brightness 0.2, contrast 0.2, saturation 0.2' in text
    losses = [float(x) for x in re.findall(r' total_loss=([-0-9.naninf]+)', text)]
    assert len(losses) >= 2 and all(np.isfinite(v) for v in losses), text[-2000:]
    ck = glob.glob(os.path.join(snap, 'epoch_0_123.pth' if ft else 'epoch_1.pth'))
    assert ck and all(torch.isfinite(v.float()).all() for v in torch.load(ck[0], map_location='cpu').values())
    n_train = 3 if ft else 16                                 # full batches of 4: 7 base classes x 2 shots = 14 pairs; 64 tiles
    assert calls['sl_augment_batch_ex'] == n_train, calls
    before = dict(calls)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        main(common + ['--snapshot-dir', str(tmp_path / 'off'), '--num-workers', '0'])
    assert calls['sl_augment_batch_ex'] == before['sl_augment_batch_ex'] and calls['sl_augment_batch'] - before['sl_augment_batch'] >= n_train, calls
    assert 'tile augmentation' not in '\n'.join(r.getMessage() for r in caplog.records)
