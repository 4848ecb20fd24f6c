"""sl_augment_batch_geo on the GPU: arbitrary-angle rotation about the crop centre and Gaussian blur in the one launch that prepares a batch (csrc/augment.hip; the contract is
the comment in include/segland_hip.h, restated in float64 by aug_geo_reference.py).  With rotate = blur_k = 0 the entry is sl_augment_batch_ex bit for bit.  With them, away
from the reference's near-tie mask (at most 2 pixels of a crop, 0.1 % overall: test_aug_rotate_cpu.py asserts that cap on these very inputs, found 160 of 655 360) labels and
padding are exact and the image holds ATOL = 7.9e-6 on the normalised values: the float32 evaluation of the reference stays within 5.3e-7 of its float64 evaluation over the
inputs of the rotation and the blur tests (computed on the CPU, asserted in test_aug_rotate_cpu.py), and 15 times that covers summation order, the two extra passes of the blur
and FMA contraction, and nothing more.  Tiles <= 64 x 64, crops 32 x 32 unless a test says otherwise."""
import glob
import logging
import os
import random
import re

import numpy as np
import pytest
import torch

import aug_geo_cases as gc
import aug_geo_reference as gr
import aug_reference as ar

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CH, CW = gc.CH, gc.CW
MEAN, STD, LUT = gc.MEAN, gc.STD, gc.LUT
ATOL = 7.9e-6
PAD_VALUE = (0.0 - np.array(MEAN)) / np.array(STD)


def _geo(d):
    from segland_amd.dataset.augment import GeoDraw
    return GeoDraw(*d)


def _augmenter(lut=None, crop=(CH, CW), mean=MEAN, std=STD):
    from segland_amd.dataset.augment import TileAugmenter
    return TileAugmenter(crop, mean, std, 255, lut=lut, device=DEV)


def _against_reference(aug, tiles, cases, crop, lut, what):
    """One launch of `cases` = [(tile index, 16-tuple)]; labels, padding and padding values exact and the image within ATOL away from the near-tie mask.
    -> (max image error, near-tie pixels, padding pixels, inside pixels, kernel labels)."""
    got_i, got_l = aug.prepare([tiles[t] for t, _ in cases], [_geo(d) for _, d in cases])
    got_i, got_l = got_i.cpu().numpy().astype(np.float64), got_l.cpu().numpy()
    worst, nt, npad, nin = 0.0, 0, 0, 0
    for j, (t, d) in enumerate(cases):
        want_i, want_l, pad, tie = gr.prepare(tiles[t][0], tiles[t][1], d, crop, MEAN, STD, 255, lut)
        free = ~tie
        assert int(tie.sum()) <= 2, (what, j, d)
        assert np.array_equal(got_l[j][free], want_l[free]), (what, j, d)
        assert np.array_equal((got_l[j] == 255)[free], pad[free]), (what, j, d)      # the table maps no label to 255: the kernel's padding mask, exactly
        assert np.array_equal(got_i[j][:, free & pad], np.broadcast_to(PAD_VALUE[:, None], (3, int((free & pad).sum())))), (what, j, d)      # 0 before normalisation, exactly
        worst = max(worst, float(np.abs(got_i[j] - want_i)[:, free].max()))
        nt, npad, nin = nt + int(tie.sum()), npad + int(pad.sum()), nin + int((~pad).sum())
    return worst, nt, npad, nin, got_l


# --------------------------------------------------------------------------------------------- rotate = 0, blur_k = 0: sl_augment_batch_ex bit for bit
@pytest.mark.parametrize('lut', [None, LUT], ids=['nolut', 'lut'])
def test_no_rotation_no_blur_equals_the_ex_entry_bit_for_bit(hip, lut):
    from segland_amd.dataset.augment import ExtDraw
    tiles = gc.tiles(1)
    aug = _augmenter(lut)
    batch, ext, geo = [], [], []
    for flip in (False, True):
        for k in range(4):
            for t, (img, lab) in enumerate(tiles):
                H, W = lab.shape
                s = gc.SCALES[(t + k) % len(gc.SCALES)]
                Hs, Ws = ar.scaled_size(H, s), ar.scaled_size(W, s)
                mh, mw = max(Hs - CH, 0), max(Ws - CW, 0)
                for h_off, w_off in {(0, 0), (mh, mw), (mh // 2, mw // 3)}:
                    d = gr.angle_draw(h_off, w_off, flip, k, Hs, Ws, gc.STRONG if (t + k) % 2 else None, H)
                    batch.append((img, lab))
                    ext.append(ExtDraw(*d[:12]))
                    geo.append(_geo(d))
    want_i, want_l = aug.prepare(batch, ext)
    got_i, got_l = aug.prepare(batch, geo)
    assert torch.equal(got_i, want_i) and torch.equal(got_l, want_l)
    assert (want_l == 255).any() and len(batch) >= 8 * 4


def test_no_rotation_no_blur_of_unlabeled_tiles(hip):
    from segland_amd.dataset.augment import ExtDraw
    tiles = [(img, None) for img, _ in gc.tiles(2)]
    aug = _augmenter()
    draws = [gr.angle_draw(i % 3, (2 * i) % 5, bool(i % 2), i % 4, t[0].shape[0], t[0].shape[1], None, t[0].shape[0]) for i, t in enumerate(tiles)]
    want_i, want_l = aug.prepare(tiles, [ExtDraw(*d[:12]) for d in draws])
    got_i, got_l = aug.prepare(tiles, [_geo(d) for d in draws])
    assert want_l is None and got_l is None and torch.equal(got_i, want_i)
    rot_i, rot_l = aug.prepare(tiles, [_geo(gr.angle_draw(1, 2, False, i % 4, t[0].shape[0], t[0].shape[1], None, t[0].shape[0], 61.3, 5)) for i, t in enumerate(tiles)])
    assert rot_l is None and torch.isfinite(rot_i).all()


def test_a_mixed_batch_equals_the_per_kind_results(hip):
    """Plain draws, ExtDraws and GeoDraws in one batch go through the new entry as a whole; every tile comes out as its own kind's launch prepares it."""
    from segland_amd.dataset.augment import ExtDraw
    tiles = gc.tiles(4)
    aug = _augmenter(LUT)
    batch, draws = [], []
    for i in range(12):
        t = i % len(tiles)
        H, W = tiles[t][1].shape
        Hs, Ws = ar.scaled_size(H, 1.37), ar.scaled_size(W, 1.37)
        batch.append(tiles[t])
        draws.append([(i % 3, i % 5, bool(i % 2), i % 4), ExtDraw(*gr.angle_draw(3, 4, bool(i % 2), i % 4, Hs, Ws, gc.STRONG, H)[:12]),
                      _geo(gr.angle_draw(3, 4, bool(i % 2), i % 4, Hs, Ws, gc.STRONG, H, gc.ANGLES[i % 5], (0, 5, 11)[i % 3]))][i % 3])
    got_i, got_l = aug.prepare(batch, draws)
    for kind in range(3):
        idx = list(range(kind, 12, 3))
        want_i, want_l = aug.prepare([batch[i] for i in idx], [draws[i] for i in idx])
        assert torch.equal(got_i[idx], want_i) and torch.equal(got_l[idx], want_l), kind


# --------------------------------------------------------------------------------------------- rotation against the float64 reference
@pytest.mark.parametrize('triple', [None, gc.STRONG], ids=['nojitter', 'strong'])
def test_rotation_matches_the_float64_reference(hip, triple):
    """4 tiles (one smaller than the crop) x 5 launches in which every tile meets every scale and every angle x flip x k x offsets at 0 and at the far edge."""
    tiles = gc.tiles(3)
    aug = _augmenter(LUT)
    worst, ties, total = 0.0, 0, 0
    for n, cases in enumerate(gc.rotation_launches(triple)):
        w, nt, npad, nin, _ = _against_reference(aug, tiles, cases, (CH, CW), LUT, 'launch %d' % n)
        assert npad > 0 and nin > 0
        worst, ties, total = max(worst, w), ties + nt, total + npad + nin
    print('rotation %s: max |kernel - float64 reference| on the normalised image %.3g (bound %.1e); %d of %d pixels in the near-tie mask' % (triple, worst, ATOL, ties, total))
    assert ties <= 1e-3 * total
    assert worst <= ATOL


def test_angle_zero_with_the_rotation_on(hip):
    """cos = 1, sin = 0: the double chain is exact, ties included -- labels and padding equal the rotate = 0 launch, the image is within ATOL of it."""
    tiles = gc.tiles(5)
    aug = _augmenter(LUT)
    batch, on, off = [], [], []
    for t, (img, lab) in enumerate(tiles):
        H, W = lab.shape
        for i, s in enumerate(gc.SCALES):
            Hs, Ws = ar.scaled_size(H, s), ar.scaled_size(W, s)
            for h_off, w_off in ((0, 0), (max(Hs - CH, 0), max(Ws - CW, 0))):
                batch.append((img, lab))
                on.append(_geo(gr.angle_draw(h_off, w_off, bool(i % 2), (t + i) % 4, Hs, Ws, None, H, 0.0)))
                off.append(_geo(gr.angle_draw(h_off, w_off, bool(i % 2), (t + i) % 4, Hs, Ws, None, H)))
    a_i, a_l = aug.prepare(batch, on)
    b_i, b_l = aug.prepare(batch, off)
    assert torch.equal(a_l, b_l)
    pad = torch.as_tensor(PAD_VALUE, dtype=torch.float32, device=DEV)[None, :, None, None]
    assert torch.equal((a_i == pad).all(1), (b_i == pad).all(1)) and (b_l == 255).any()
    worst = float((a_i.double() - b_i.double()).abs().max())
    print('angle 0: max |rotate = 1 - rotate = 0| %.3g' % worst)
    assert worst <= ATOL


# --------------------------------------------------------------------------------------------- blur against the reference
def test_blur_matches_the_float64_reference(hip):
    tiles = gc.tiles(7)
    worst = 0.0
    for name, crop, cases in gc.blur_launches():
        aug = _augmenter(LUT, crop)
        w, _, npad, nin, got_l = _against_reference(aug, tiles, cases, crop, LUT, name)
        assert nin > 0 and (npad > 0 or crop == (8, 8))       # padding taps and padding outputs in every launch but the 8 x 8 one, which lies inside every tile
        # labels are never blurred: the same launch without the blur gives the same labels, and another image
        plain_i, plain_l = aug.prepare([tiles[t] for t, _ in cases], [_geo(d[:15] + (0,)) for _, d in cases])
        assert np.array_equal(plain_l.cpu().numpy(), got_l)
        print('blur %s on %dx%d: max |kernel - float64 reference| %.3g (bound %.1e)' % ((name,) + tuple(crop) + (w, ATOL)))
        worst = max(worst, w)
    assert worst <= ATOL


def test_blur_and_the_strongest_jitter_stay_in_range(hip):
    """The all-255 and all-0 tiles of the clip test under an 11-tap blur and the strongest triple, and its mirror images."""
    aug = _augmenter()
    worst = 0.0
    for triple in ((1.99, 0.5, 1.99), (1.99, -0.5, 1.99), (0.01, 0.5, 0.01)):
        tiles, cases = [], []
        for value in (255, 0):
            tiles.append((np.full((40, 56, 3), value, dtype=np.uint8), np.zeros((40, 56), dtype=np.uint8)))
        mixed = np.zeros((40, 56, 3), dtype=np.uint8)
        mixed[:, :, 0] = 255
        tiles.append((mixed, np.zeros((40, 56), dtype=np.uint8)))
        for t in range(3):
            cases.append((t, gr.angle_draw(5, 7, t == 2, 2 * (t == 2), 55, 77, triple, 40, (None, -33.0, 7.5)[t], 11)))
        got = aug.prepare(tiles, [_geo(d) for _, d in cases])[0].cpu().numpy().astype(np.float64)
        assert got.min() >= -1.0 and got.max() <= 1.0
        for j, (t, d) in enumerate(cases):
            want = gr.prepare(tiles[t][0], tiles[t][1], d, (CH, CW), MEAN, STD)[0]
            assert want.min() >= -1.0 - 1e-12 and want.max() <= 1.0 + 1e-12
            worst = max(worst, float(np.abs(got[j] - want).max()))
    print('blur + clip saturation: max |kernel - float64 reference| %.3g' % worst)
    assert worst <= ATOL


def test_two_runs_give_the_same_bits(hip):
    tiles = gc.tiles(4)
    aug = _augmenter()
    draws = [_geo(gr.angle_draw(3, 4, bool(t % 2), t, ar.scaled_size(l.shape[0], 1.37), ar.scaled_size(l.shape[1], 1.37), gc.STRONG, l.shape[0], gc.ANGLES[t], gc.BLUR_SIZES[t]))
             for t, (_, l) in enumerate(tiles)]
    a, b = aug.prepare(tiles, draws), aug.prepare(tiles, draws)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# --------------------------------------------------------------------------------------------- row slicing in the workers' collate
def test_row_sliced_packed_tiles_prepare_identically(hip):
    """The same batch as a list of whole arrays, packed whole (RawCollate(None)) and packed after the collate cut every tile down to the rows source_rows_geo names."""
    from segland_amd.dataset.oem import PackedTiles, RawCollate
    tiles = gc.tiles(6)[:3]
    aug = _augmenter()
    draws, batch = [], []
    for n in range(len(gc.SCALES)):
        for t, (img, lab) in enumerate(tiles):
            H, W = lab.shape
            s = gc.SCALES[(n + t) % len(gc.SCALES)]
            Hs, Ws = ar.scaled_size(H, s), ar.scaled_size(W, s)
            for edge in (0, 1, 2):
                h_off, w_off = (0, 0) if edge == 0 else (max(Hs - CH, 0) // (3 - edge), max(Ws - CW, 0) // (3 - edge))
                draws.append(_geo(gr.angle_draw(h_off, w_off, bool(edge % 2), (n + edge) % 4, Hs, Ws, gc.STRONG if edge else None, H, (7.5, -7.5, None)[edge], (0, 5, 11)[(n + edge) % 3])))
                batch.append((img, lab))
    draws.append((2, 3, True, 3))                             # a plain draw among them
    batch.append(tiles[2])
    want_i, want_l = aug.prepare(batch, draws)
    samples = [(b[0], b[1], d, i) for i, (b, d) in enumerate(zip(batch, draws))]
    whole, pw, _ = RawCollate(None)(samples)
    cut, pc, _ = RawCollate(CH)(samples)
    assert isinstance(cut, PackedTiles) and cut.buf.numel() < whole.buf.numel()
    assert any(p.row0 > 0 and p.rotate for p in pc[:-1]) and all(cut[i][0].shape[0] <= batch[i][0].shape[0] for i in range(len(batch)))
    for packed, prm in ((whole, pw), (cut, pc)):
        got_i, got_l = aug.prepare(packed, prm)
        assert torch.equal(got_i, want_i) and torch.equal(got_l, want_l)


# --------------------------------------------------------------------------------------------- what the Python side refuses, and the C side before any launch
def test_refusals_before_any_launch(hip, monkeypatch):
    from segland_amd import _lib
    from segland_amd.dataset.augment import TileAugmenter
    from segland_amd.ops import _p, _s
    lib = _lib.lib()
    launches = []
    real = lib.sl_augment_batch_geo
    monkeypatch.setattr(lib, 'sl_augment_batch_geo', lambda *a: launches.append(a) or real(*a))
    tiles = gc.tiles(5)[:1]
    aug = _augmenter()
    H, W = tiles[0][1].shape
    with pytest.raises(ValueError, match='reads source rows'):      # a buffer that lacks the rows the rotated crop's taps need
        aug.prepare([(tiles[0][0][:10], tiles[0][1][:10])], [_geo(gr.angle_draw(0, 0, False, 0, H, W, None, H, 33.0))])
    with pytest.raises(ValueError, match='reads source rows'):
        aug.prepare([(tiles[0][0][8:], tiles[0][1][8:])], [_geo(gr.angle_draw(4, 0, False, 0, H, W, None, H, -7.5))._replace(row0=8)])
    with pytest.raises(ValueError, match='8 x 5'):                  # a crop side <= R
        TileAugmenter((8, 5), MEAN, STD, 255, device=DEV).prepare(tiles, [_geo(gr.angle_draw(0, 0, False, 0, H, W, None, H, None, 11))])
    with pytest.raises(ValueError, match='blur size'):
        aug.prepare(tiles, [_geo(gr.angle_draw(0, 0, False, 0, H, W, None, H, None, 4))])
    with pytest.raises(ValueError, match='cosine'):
        aug.prepare(tiles, [_geo(gr.angle_draw(0, 0, False, 0, H, W, None, H, 10.0))._replace(cos_t=float('nan'))])
    with pytest.raises(ValueError, match='square'):
        TileAugmenter((32, 16), MEAN, STD, 255, device=DEV).prepare(tiles, [_geo(gr.angle_draw(0, 0, False, 1, H, W, None, H, 10.0))])
    assert not launches
    out = torch.empty((1, 3, CH, CW), device=DEV)
    table = torch.zeros(128, dtype=torch.uint8, device=DEV)
    for args in ((None, 1, CH, CW, aug.mean, aug.std, _p(out)), (_p(table), 0, CH, CW, aug.mean, aug.std, _p(out)), (_p(table), 1, 0, CW, aug.mean, aug.std, _p(out)),
                 (_p(table), 1, CH, -1, aug.mean, aug.std, _p(out)), (_p(table), 1, CH, CW, None, aug.std, _p(out)), (_p(table), 1, CH, CW, aug.mean, None, _p(out)),
                 (_p(table), 1, CH, CW, aug.mean, aug.std, None), (_p(table), 65536, CH, CW, aug.mean, aug.std, _p(out))):
        t, B, ch, cw, m, s, o = args
        assert real(t, B, ch, cw, m, s, 255, None, o, None, _s()) != 0


# --------------------------------------------------------------------------------------------- pairs
def test_pair_augmenter_with_all_four_options_equals_the_reference_per_tile(hip):
    from segland_amd.dataset import oem_ft, synthetic_raw_ft
    from segland_amd.dataset.augment import GeoDraw
    random.seed(11)
    np.random.seed(11)
    ds = synthetic_raw_ft.GFSSegTrain(crop_size=(CH, CW), shot=2, length=12, tile=(60, 64),
                                      augment={'scale': (0.5, 2.0), 'jitter': (0.3, 0.3, 0.3), 'rotate': (-180.0, 180.0, 1.0), 'blur': (5, 1.0)})
    samples = [ds[0], ds[5]]
    packed, params, _ = ds.collate_fn(samples)
    img, mask, img_b, mask_b = ds.augmenter(DEV).prepare(packed, params)
    assert img.shape == (2, 3, CH, CW) and mask_b.dtype == torch.int64
    worst = 0.0
    for i, ((nov, base), (pn, pb), _) in enumerate(samples):
        assert type(pn) is GeoDraw and type(pb) is GeoDraw and pn != pb and pn.rotate and pb.blur_k == 5
        for (tile, d, gi, gl) in ((nov, pn, img[i], mask[i]), (base, pb, img_b[i], mask_b[i])):
            want_i, want_l, _, tie = gr.prepare(tile[0], tile[1], tuple(d), (CH, CW), oem_ft.MEAN, oem_ft.STD, 255)
            assert int(tie.sum()) <= 2 and np.array_equal(gl.cpu().numpy()[~tie], want_l[~tie])
            worst = max(worst, float(np.abs(gi.cpu().numpy().astype(np.float64) - want_i)[:, ~tie].max()))
    # ImageNet statistics divide by std >= 0.224 where the bound was worked out for 0.5
    bound = ATOL * 0.5 / min(oem_ft.STD)
    print('pairs: max |kernel - float64 reference| on the normalised image (ImageNet statistics) %.3g (bound %.2e)' % (worst, bound))
    assert worst <= bound


# --------------------------------------------------------------------------------------------- drivers
def _count_calls(monkeypatch):
    from segland_amd import _lib
    lib = _lib.lib()
    calls = {'sl_augment_batch': 0, 'sl_augment_batch_ex': 0, 'sl_augment_batch_geo': 0}
    for name in calls:
        fn = getattr(lib, name)

        def wrapper(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapper)
    return calls


@pytest.mark.parametrize('ft', [False, True], ids=['train_base', 'ft_pop'])
def test_drivers_train_with_the_rotation_and_blur_flags(hip, tmp_path, caplog, monkeypatch, ft):
    """One short epoch on synthetic_raw with both flags at probability 1: finite losses and weights, the start-up line, every training batch through the new entry; the same
    run without the flags never reaches it."""
    from segland_amd import ft_pop, train_base
    calls = _count_calls(monkeypatch)
    common = ['--model', 'pspnet_pop', '--backbone', 'resnet50', '--dataset', 'synthetic_raw', '--input-size', '128,128', '--base-size', '128,128', '--num-epoch', '1',
              '--restore-from', '/nonexistent', '--allow-random-init']
    common += (['--batch-size', '4', '--learning-rate', '1e-3', '--print-frequency', '1', '--random-seed', '123', '--freeze-backbone', '--fix-bn', '--shot', '2'] if ft
               else ['--batch-size', '4', '--learning-rate', '1e-4', '--print-frequency', '4', '--fp16'])
    main = ft_pop.main if ft else train_base.main
    snap = str(tmp_path / 'on')
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        main(common + ['--snapshot-dir', snap, '--num-workers', '2', '--aug-rotate=-180,180,1', '--aug-blur', '5,1'])
    text = '\n'.join(r.getMessage() for r in caplog.records)
    assert 'rotation by -180..180 degrees about the crop centre (probability 1)' in text and '5x5 Gaussian blur (probability 1)' in text
    losses = [float(x) for x in re.findall(r' total_loss=([-0-9.naninf]+)', text)]
    assert len(losses) >= 2 and all(np.isfinite(v) for v in losses), text[-2000:]
    ck = glob.glob(os.path.join(snap, 'epoch_0_123.pth' if ft else 'epoch_1.pth'))
    assert ck and all(torch.isfinite(v.float()).all() for v in torch.load(ck[0], map_location='cpu').values())
    n_train = 3 if ft else 16                                 # full batches of 4: 7 base classes x 2 shots = 14 pairs; 64 tiles
    assert calls['sl_augment_batch_geo'] == n_train and calls['sl_augment_batch_ex'] == 0, calls
    before = dict(calls)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        main(common + ['--snapshot-dir', str(tmp_path / 'off'), '--num-workers', '0'])
    assert calls['sl_augment_batch_geo'] == before['sl_augment_batch_geo'] and calls['sl_augment_batch_ex'] == 0 and calls['sl_augment_batch'] - before['sl_augment_batch'] >= n_train, calls
    assert 'tile augmentation' not in '\n'.join(r.getMessage() for r in caplog.records)
