"""Random rescale + colour jitter of the tile feed, the parts that need no GPU: the float64 reference of the GPU tests (aug_reference.py) against torch's own interpolate where
the conventions coincide, the host draws (order, rounding, ranges, the redraw on the SAMPLED label window, no new random numbers with the options off), the row slicing helper
against brute force, and the two command-line flags in both parsers."""
import random
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aug_reference as ar

TILES = [(40, 56), (37, 53), (64, 64)]
SCALES = [0.5, 0.73, 1.0, 1.37, 2.0, 3.99]


def _tile(h, w, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8), rng.randint(0, 12, (h, w)).astype(np.uint8)


@pytest.mark.parametrize('hw', TILES)
@pytest.mark.parametrize('s', SCALES)
def test_reference_resample_against_torch(hw, s):
    h, w = hw
    img, lbl = _tile(h, w, 11)
    Hs, Ws = ar.scaled_size(h, s), ar.scaled_size(w, s)
    got = ar.resample(img, Hs, Ws)
    want = F.interpolate(torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None], size=(Hs, Ws), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).numpy()
    diff = float(np.abs(got - want).max())
    print('resample %dx%d x %g -> %dx%d: max |reference - torch| %.3g' % (h, w, s, Hs, Ws, diff))
    assert diff <= 1e-9
    if s == 1.0:
        assert np.array_equal(got, img.astype(np.float64))
        assert np.array_equal(ar.resample_label(lbl, Hs, Ws), lbl)


@pytest.mark.parametrize('hw', TILES)
@pytest.mark.parametrize('s', SCALES)
def test_reference_labels_against_torch_away_from_ties(hw, s):
    """torch's nearest-exact computes floor((i + 0.5) * scale) in floating point; where the pixel centre falls exactly on a source pixel border its product lands on either
    side.  Away from those ties the two must agree; on them the integer rule is checked against exact rational arithmetic."""
    h, w = hw
    _, lbl = _tile(h, w, 12)
    Hs, Ws = ar.scaled_size(h, s), ar.scaled_size(w, s)
    got = ar.resample_label(lbl, Hs, Ws)
    want = F.interpolate(torch.from_numpy(lbl.astype(np.float64))[None, None], size=(Hs, Ws), mode='nearest-exact')[0, 0].numpy().astype(np.uint8)
    ty, tx = ar.tie(np.arange(Hs), h, Hs), ar.tie(np.arange(Ws), w, Ws)
    free = ~ty[:, None] & ~tx[None, :]
    assert np.array_equal(got[free], want[free])
    print('labels %dx%d x %g: %d tied pixels, %d of them differ from torch' % (h, w, s, int((~free).sum()), int((got != want).sum())))
    for P, S, Ss, tied in ((np.arange(Hs), h, Hs, ty), (np.arange(Ws), w, Ws, tx)):
        idx = ar.taps(P, S, Ss)[3]
        for p in P:
            centre = Fraction((2 * int(p) + 1) * S, 2 * Ss)          # (p + 1/2) S / Ss: the source coordinate of the pixel centre, pixel j covering [j, j + 1)
            assert int(idx[p]) == min(centre.numerator // centre.denominator, S - 1)
            assert bool(tied[p]) == (centre.denominator == 1)
            if tied[p]:
                assert int(idx[p]) == min(int(centre), S - 1)         # a tie goes to the pixel that starts there


def test_a_tied_case_exists():
    """64 -> 47 (scale 0.73): row 23 sits exactly between source rows 31 and 32, so the tie branch above is exercised."""
    assert ar.scaled_size(64, 0.73) == 47 and ar.tie(np.arange(47), 64, 47).tolist().count(True) == 1 and bool(ar.tie(23, 64, 47))


# ------------------------------------------------------------------------------------------------------------------------------------------------ draws
def _draw_before_this_option(label, crop_size, ignore_label=255, mode='train'):
    """draw_train_params as it was before scale= / jitter= existed, statement for statement."""
    H, W = label.shape
    ch, cw = crop_size
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


def _seed(n):
    random.seed(n)
    np.random.seed(n)


def _states():
    return random.getstate(), np.random.get_state()


def _same_states(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


@pytest.mark.parametrize('mode,kw', [('train', {}), ('train', {'scale': None, 'jitter': None}), ('val_supp', {}), ('val_supp', {'scale': (0.5, 2.0), 'jitter': (0.2, 0.2, 0.2)})])
def test_draws_without_the_options_are_the_old_draws(mode, kw):
    from segland_amd.dataset.augment import draw_train_params
    label = _tile(96, 80, 5)[1]
    label[:60] = 255                                      # most windows near the top are all-ignore: the redraw loop runs
    for seed in range(6):
        _seed(seed)
        want = [_draw_before_this_option(label, (32, 32), 255, mode) for _ in range(5)]
        after_want = _states()
        _seed(seed)
        got = [draw_train_params(label, (32, 32), 255, mode, **kw) for _ in range(5)]
        assert got == want and all(type(g) is tuple and len(g) == 4 for g in got)
        assert _same_states(_states(), after_want)


def test_extended_draws_order_rounding_and_ranges():
    from segland_amd.dataset.augment import draw_train_params
    label = _tile(70, 90, 6)[1]
    ch = cw = 32
    lo, hi, b, c, s = 0.3, 2.0, 0.2, 0.3, 0.4
    for seed in range(40):
        _seed(seed)
        d = draw_train_params(label, (ch, cw), 255, 'train', scale=(lo, hi), jitter=(b, c, s))
        after = _states()
        _seed(seed)
        assert draw_train_params(label, (ch, cw), 255, 'train', scale=(lo, hi), jitter=(b, c, s)) == d        # seeded calls agree
        # the same numbers drawn by hand, in the documented order
        _seed(seed)
        f = random.uniform(lo, hi)
        Hs, Ws = max(1, int(70 * f + 0.5)), max(1, int(90 * f + 0.5))
        h_off, w_off = np.random.randint(0, max(Hs - ch, 0) + 1), np.random.randint(0, max(Ws - cw, 0) + 1)      # no ignore labels in this tile: accepted at once
        flip, k = random.random() < 0.5, int(random.random() // 0.25)
        alpha, beta, sigma = 1.0 + random.uniform(-c, c), random.uniform(-b, b), 1.0 + random.uniform(-s, s)
        assert _same_states(_states(), after)
        assert tuple(d[:10]) == (h_off, w_off, flip, k, Hs, Ws, 1, alpha, beta, sigma) and len(d) > 4
        assert (d.H, d.row0) == (70, 0)
        assert 0 <= d.h_off <= max(d.Hs - ch, 0) and 0 <= d.w_off <= max(d.Ws - cw, 0)
        assert 1 - c <= d.alpha <= 1 + c and -b <= d.beta <= b and 1 - s <= d.sigma <= 1 + s
    # one option alone
    _seed(3)
    d = draw_train_params(label, (ch, cw), 255, 'train', scale=(2.0, 2.0))
    assert (d.Hs, d.Ws, d.jitter, d.alpha, d.beta, d.sigma) == (140, 180, 0, 1.0, 0.0, 1.0)
    _seed(3)
    d = draw_train_params(label, (ch, cw), 255, 'train', jitter=(0.1, 0.1, 0.1))
    assert (d.Hs, d.Ws, d.jitter) == (70, 90, 1)
    assert ar.scaled_size(37, 0.5) == 19 and ar.scaled_size(1, 0.3) == 1        # int(H s + 0.5), never below 1


def test_redraw_looks_at_the_sampled_label_window():
    """At scale 0.5 of an even tile nearest sampling reads source index 2Y + 1 only.  The label is valid on every even row and column (never read) and at the single odd
    pixel (63, 63): only the crop that holds rescaled pixel (31, 31) -- offsets (16, 16) -- is not all-ignore as the kernel will see it, while EVERY 16 x 16 window of the
    source label holds valid pixels."""
    from segland_amd.dataset.augment import draw_train_params
    label = np.full((64, 64), 255, dtype=np.uint8)
    label[::2, :] = 3
    label[:, ::2] = 4
    label[63, 63] = 5
    assert (ar.resample_label(label, 32, 32) != 255).sum() == 1
    for seed in range(3):
        _seed(seed)
        d = draw_train_params(label, (16, 16), 255, 'train', scale=(0.5, 0.5))
        assert (d.Hs, d.Ws, d.h_off, d.w_off) == (32, 32, 16, 16)


def test_source_rows_equals_brute_force():
    from segland_amd.dataset.augment import source_rows
    n = 0
    for H in (1, 2, 7, 37, 40, 64):
        for s in (0.26, 0.5, 0.73, 1.0, 1.37, 2.0, 3.99):
            Hs = ar.scaled_size(H, s)
            for ch in (1, 5, 32):
                offs = sorted({0, max(Hs - ch, 0), max(Hs - ch, 0) // 2, min(3, Hs - 1), Hs - 1})
                for h_off in offs:
                    got = source_rows(H, Hs, h_off, ch)
                    assert got == ar.source_rows_brute(H, Hs, h_off, ch), (H, Hs, h_off, ch)
                    assert 0 <= got[0] and got[0] + got[1] <= H and got[1] >= 1
                    n += 1
    assert any(ar.scaled_size(H, 0.5) < 32 for H in (37, 40)) and n > 300


def test_crop_rows_slices_extended_draws_and_leaves_plain_ones_as_they_were():
    from segland_amd.dataset.augment import ExtDraw, source_rows
    from segland_amd.dataset.oem import crop_rows
    img, lab = _tile(64, 48, 9)
    d = ExtDraw(70, 3, True, 1, 128, 96, 0, 1.0, 0.0, 1.0, 64, 0)
    ci, cl, cd = crop_rows(img, lab, d, 32)
    row0, rows = source_rows(64, 128, 70, 32)
    assert cd == d._replace(row0=row0) and ci.shape[0] == rows < 64 and np.array_equal(ci, img[row0:row0 + rows]) and np.array_equal(cl, lab[row0:row0 + rows])
    assert crop_rows(img, lab, d, None)[2] == d and crop_rows(img, lab, d, None)[0] is img
    pi, pl, pd = crop_rows(img, lab, (10, 3, True, 1), 32)
    assert pd == (0, 3, True, 1) and np.array_equal(pi, img[10:42]) and np.array_equal(pl, lab[10:42])


# ------------------------------------------------------------------------------------------------------------------------------------------------ command line
@pytest.mark.parametrize('ft', [False, True])
def test_parsers_accept_and_refuse_the_augmentation_flags(ft, capsys):
    from segland_amd.drivers import build_parser
    p = build_parser(ft)
    a = p.parse_args([])
    assert a.aug_scale == () and a.aug_jitter == ()
    a = p.parse_args(['--aug-scale', '0.5,2.0', '--aug-jitter', '0.2,0.1,0'])
    assert a.aug_scale == (0.5, 2.0) and a.aug_jitter == (0.2, 0.1, 0.0)
    assert p.parse_args(['--aug-scale', '1,1']).aug_scale == (1.0, 1.0) and p.parse_args(['--aug-scale', '0.25,4']).aug_scale == (0.25, 4.0)
    assert p.parse_args(['--aug-scale', '']).aug_scale == () and p.parse_args(['--aug-jitter', '']).aug_jitter == ()
    for flag, bad in [('--aug-scale', '0,2'), ('--aug-scale', '2,0.5'), ('--aug-scale', '0.5,4.5'), ('--aug-scale', '0.5'), ('--aug-scale', '0.5,1,2'), ('--aug-scale', 'a,b'),
                      ('--aug-scale', 'nan,1'), ('--aug-scale=-1,2', None), ('--aug-jitter', '0.2,0.2'), ('--aug-jitter', '1,0,0'), ('--aug-jitter', '0.2,0.2,1.5'),
                      ('--aug-jitter=-0.1,0,0', None), ('--aug-jitter', 'x,0,0'), ('--aug-jitter', '0.1,nan,0')]:
        with pytest.raises(SystemExit):
            p.parse_args([flag] if bad is None else [flag, bad])
        err = capsys.readouterr().err
        assert (bad if bad is not None else flag.split('=')[1]) in err, err        # the message holds the value


def test_a_reader_without_raw_tiles_refuses_the_flags_by_name():
    from segland_amd.drivers import augment_option, build_parser
    from segland_amd.dataset import synthetic, synthetic_ft, synthetic_raw, synthetic_raw_ft, synthetic_tiff, synthetic_tiff_ft, oem, oem_ft
    off = build_parser(False).parse_args([])
    assert augment_option(off, synthetic.GFSSegTrain, 'synthetic') == {}                       # flags off: the reader is called as it always was
    for ft, mod, name in ((False, synthetic, 'synthetic'), (True, synthetic_ft, 'synthetic_ft')):
        for argv, flag in ((['--aug-scale', '0.5,2'], '--aug-scale'), (['--aug-jitter', '0.2,0.2,0.2'], '--aug-jitter')):
            with pytest.raises(ValueError) as e:
                augment_option(build_parser(ft).parse_args(argv), mod.GFSSegTrain, name)
            assert name in str(e.value) and flag in str(e.value)
    on = build_parser(False).parse_args(['--aug-scale', '0.5,2', '--aug-jitter', '0.2,0.2,0.2'])
    for mod in (synthetic_raw, synthetic_raw_ft, synthetic_tiff, synthetic_tiff_ft, oem, oem_ft):
        assert augment_option(on, mod.GFSSegTrain, 'x') == {'augment': {'scale': (0.5, 2.0), 'jitter': (0.2, 0.2, 0.2)}}
    assert augment_option(build_parser(True).parse_args(['--aug-scale', '0.5,2']), oem.GFSSegTrain, 'x') == {'augment': {'scale': (0.5, 2.0), 'jitter': None}}


def test_the_log_line_appears_only_with_a_flag(caplog):
    import logging
    from segland_amd.drivers import build_parser, log_augment_options
    with caplog.at_level(logging.INFO, logger='Segmentation'):
        log_augment_options(build_parser(False).parse_args([]))
        assert not caplog.records
        log_augment_options(build_parser(True).parse_args(['--aug-scale', '0.5,2']))
        log_augment_options(build_parser(False).parse_args(['--aug-scale', '0.5,2', '--aug-jitter', '0.2,0.1,0.3']))
    msgs = [r.getMessage() for r in caplog.records]
    assert len(msgs) == 2 and '0.5..2' in msgs[0] and 'jitter' not in msgs[0] and 'brightness 0.2, contrast 0.1, saturation 0.3' in msgs[1]


def test_readers_hand_the_ranges_to_the_draws():
    """synthetic_raw / synthetic_raw_ft with augment= emit extended draws (both tiles of a pair their own), without it the plain 4-tuples; validation readers have no such
    option."""
    import inspect
    from segland_amd.dataset import oem, synthetic_raw, synthetic_raw_ft
    aug = {'scale': (0.5, 2.0), 'jitter': (0.2, 0.2, 0.2)}
    _seed(1)
    ds = synthetic_raw.GFSSegTrain(crop_size=(32, 32), length=4, augment=aug)
    d = ds[1][2]
    assert len(d) > 4 and d.jitter == 1 and (d.H, d.row0) == (128, 0) and 64 <= d.Hs <= 256
    assert len(synthetic_raw.GFSSegTrain(crop_size=(32, 32), length=4)[1][2]) == 4
    packed, params, _ = ds.collate_fn([ds[0], ds[1]])
    assert all(len(p) > 4 and packed[i][0].shape[0] <= min(128, 32 * 128 // p.Hs + 3) for i, p in enumerate(params))
    _seed(2)
    ft = synthetic_raw_ft.GFSSegTrain(crop_size=(32, 32), shot=2, length=12, augment=aug)
    (pn, pb) = ft[0][1]
    assert len(pn) > 4 and len(pb) > 4 and (pn.Hs, pn.alpha) != (pb.Hs, pb.alpha)
    assert len(synthetic_raw_ft.GFSSegTrain(crop_size=(32, 32), shot=2, length=12)[0][1][0]) == 4
    for val in (oem.GFSSegVal, synthetic_raw.GFSSegVal):
        assert 'augment' not in inspect.signature(val.__init__).parameters
    with pytest.raises(ValueError):
        synthetic_raw.GFSSegTrain(crop_size=(32, 32), augment={'hue': 0.1})
