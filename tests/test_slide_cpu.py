"""Sliding-window inference, CPU side: sl_slide_fuse and sl_slide_windows are declared and exported, the entry point refuses every bad argument before any launch (a dummy
pointer, no device), the window grid of segland_amd/slide.py equals the formula and the exported count over a sweep, covers every pixel and stays inside the scene, and
the evaluation parser leaves sliding off by default."""
import ctypes as C
import os

import pytest

import slide_reference as sr


@pytest.fixture(scope='module')
def lib():
    from segland_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


SWEEP = [(L, c, s) for L in (1, 2, 3, 7, 9, 16, 30, 33, 40, 72, 104, 1024) for c in (1, 2, 4, 12, 16, 24, 48, 64, 512) for s in sorted({1, 2, 3, 5, c // 2, (2 * c) // 3, c - 1, c})
         if 1 <= s <= c]


def test_entry_points_are_declared_and_exported(lib):
    from segland_amd import _lib
    decl = _lib.declared_functions()
    assert 'sl_slide_fuse' in decl and len(decl['sl_slide_fuse'][1]) == 5
    assert 'sl_slide_windows' in decl and len(decl['sl_slide_windows'][1]) == 3
    assert hasattr(lib, 'sl_slide_fuse') and hasattr(lib, 'sl_slide_windows')
    header = open(_lib.HEADER).read()
    assert 'typedef struct SlSlide { int B, K, H, W, h, w, crop_h, crop_w, stride_h, stride_w, mode, blend; } SlSlide;' in header
    # the ctypes mirror has the layout of the C struct: twelve ints in the header's order
    assert C.sizeof(_lib.SlSlide) == 12 * 4
    assert [f[0] for f in _lib.SlSlide._fields_] == ['B', 'K', 'H', 'W', 'h', 'w', 'crop_h', 'crop_w', 'stride_h', 'stride_w', 'mode', 'blend']
    assert (_lib.SL_SLIDE_PROB, _lib.SL_SLIDE_LOGIT, _lib.SL_SLIDE_UNIFORM, _lib.SL_SLIDE_TENT) == (0, 1, 0, 1)
    for name, value in (('SL_SLIDE_PROB', 0), ('SL_SLIDE_LOGIT', 1), ('SL_SLIDE_UNIFORM', 0), ('SL_SLIDE_TENT', 1)):
        assert '#define %s %d' % (name, value) in header


def good(**kw):
    from segland_amd import _lib
    f = dict(B=2, K=8, H=40, W=33, h=5, w=4, crop_h=16, crop_w=12, stride_h=8, stride_w=5, mode=0, blend=0)
    f.update(kw)
    return _lib.SlSlide(**f)


def test_bad_arguments_are_refused_before_any_launch(lib):
    d = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string().decode()

    def call(desc=True, logits=d, labels=d, **kw):
        s = good(**kw)
        return lib.sl_slide_fuse(C.byref(s) if desc else None, logits, labels, None, None)

    assert call(desc=False) == -1 and 'slide_fuse' in err() and 'null' in err()
    assert call(logits=None) == -1 and 'slide_fuse' in err() and 'null' in err()
    assert call(labels=None) == -1 and 'slide_fuse' in err() and 'null' in err()
    for field in ('B', 'H', 'W', 'h', 'w', 'crop_h', 'crop_w'):
        for value in (0, -3):
            assert call(**{field: value}) == -1 and 'slide_fuse' in err() and '%s %d' % (field, value) in err(), (field, value, err())
    for kw, text in ((dict(stride_h=0), 'stride_h 0'), (dict(stride_w=-1), 'stride_w -1'), (dict(stride_h=17), 'stride_h 17'), (dict(stride_w=13), 'stride_w 13')):
        assert call(**kw) == -1 and text in err() and 'crop' in err(), (kw, err())
    assert call(K=34) == -1 and '34 logit channels' in err() and 'at most 33' in err()
    assert call(K=0) == -1 and '0 logit channels' in err()
    assert call(mode=2) == -1 and 'mode 2' in err()
    assert call(mode=-1) == -1 and 'mode -1' in err()
    assert call(blend=2) == -1 and 'blend 2' in err()
    assert call(blend=-1) == -1 and 'blend -1' in err()
    # 2^20 x 4096 x 4096 windows of one pixel do not fit an int
    assert call(B=1 << 20, H=4096, W=4096, crop_h=1, crop_w=1, stride_h=1, stride_w=1) == -1 and 'windows' in err() and str((1 << 20) * 4096 * 4096) in err()


def test_exported_window_count(lib):
    for bad in ((0, 4, 2), (-1, 4, 2), (8, 0, 1), (8, 4, 0), (8, 4, 5), (8, 4, -1)):
        assert lib.sl_slide_windows(*bad) == -1, bad
    assert lib.sl_slide_windows(8, 16, 9) == 1                       # the bound of the stride is the crop as given
    assert lib.sl_slide_windows(2 ** 31 - 1, 1, 1) == 2 ** 31 - 1
    assert lib.sl_slide_windows(1024, 512, 341) == 3


def test_window_grid_equals_the_formula_and_the_exported_count(lib):
    from segland_amd import slide
    assert len(SWEEP) > 500
    for L, c, s in SWEEP:
        side, offs = slide.window_grid(L, c, s)
        cs = min(c, L)
        n = max(L - cs + s - 1, 0) // s + 1
        assert side == cs and offs == [min(i * s, L - cs) for i in range(n)], (L, c, s)
        assert lib.sl_slide_windows(L, c, s) == len(offs), (L, c, s)
        assert (side, offs) == sr.grid(L, c, s)


def test_window_grid_covers_every_pixel_inside_the_scene():
    from segland_amd import slide
    for L, c, s in SWEEP:
        side, offs = slide.window_grid(L, c, s)
        assert offs[0] == 0 and offs[-1] == L - side and all(0 <= o and o + side <= L for o in offs), (L, c, s)
        assert offs == sorted(offs)                                  # monotone: the covering windows of a pixel are a contiguous index range
        assert all(b - a <= side for a, b in zip(offs, offs[1:])), (L, c, s)            # no hole between neighbours
        covered = set()
        for o in offs:
            covered.update(range(o, o + side))
        assert covered == set(range(L)), (L, c, s)


def test_window_grid_of_the_case_table():
    from segland_amd import slide
    for name, (K, size, crop, stride, hw, (ys, xs)) in sr.CASES.items():
        assert slide.window_grid(size[0], crop[0], stride[0]) == (min(crop[0], size[0]), ys), name
        assert slide.window_grid(size[1], crop[1], stride[1]) == (min(crop[1], size[1]), xs), name
    assert slide.window_grid(1024, 512, 341) == (512, [0, 341, 512])
    assert slide.window_grid(136, 96, 40) == (96, [0, 40]) and slide.window_grid(200, 128, 72) == (128, [0, 72])


def test_window_grid_refuses_bad_arguments():
    from segland_amd import slide
    for bad in ((0, 4, 2), (8, 0, 1), (8, 4, 0), (8, 4, 5), (8, 4, -1)):
        with pytest.raises(ValueError):
            slide.window_grid(*bad)


def test_windows_are_slices_in_index_order():
    import torch
    from segland_amd import slide
    img = torch.arange(2 * 3 * 9 * 7, dtype=torch.float32).reshape(2, 3, 9, 7)
    win = slide.windows(img, (4, 5), (3, 2))
    ys, xs = [0, 3, 5], [0, 2]
    assert tuple(win.shape) == (2 * 3 * 2, 3, 4, 5) and win.is_contiguous()
    for b in range(2):
        for iy, y in enumerate(ys):
            for ix, x in enumerate(xs):
                assert torch.equal(win[(b * 3 + iy) * 2 + ix], img[b, :, y:y + 4, x:x + 5])
    assert torch.equal(slide.windows(img, (16, 16), (16, 16)), img)          # a crop above the scene: one window, the scene itself


def test_predict_chunks_the_forwards(monkeypatch):
    """predict forwards the windows in chunks of `batch` in index order and hands ONE [N,K,h,w] tensor to the op (a stand-in model and op on the CPU: plumbing only)."""
    import torch
    from segland_amd import ops, slide
    img = torch.arange(2 * 3 * 9 * 7, dtype=torch.float32).reshape(2, 3, 9, 7)
    seen, got = [], {}

    def model(x):
        seen.append(x.shape[0])
        return x[:, :, ::2, ::2] * 2.0

    def op(logits, B, size, crop, stride, mode='prob', blend='uniform', want_map=False):
        got.update(logits=logits, B=B, size=tuple(size), crop=tuple(crop), stride=tuple(stride), mode=mode, blend=blend, want_map=want_map)
        return 'labels', None
    monkeypatch.setattr(ops, 'slide_fuse', op)
    assert slide.predict(model, img, (4, 5), (3, 2), mode='logit', blend='tent', want_map=True, batch=5) == ('labels', None)
    assert seen == [5, 5, 2]
    assert torch.equal(got.pop('logits'), slide.windows(img, (4, 5), (3, 2))[:, :, ::2, ::2] * 2.0)
    assert got == dict(B=2, size=(9, 7), crop=(4, 5), stride=(3, 2), mode='logit', blend='tent', want_map=True)
    del seen[:]
    slide.predict(model, img, (4, 5), (3, 2))
    assert seen == [12]


def test_parse_pair():
    from segland_amd import slide
    assert slide.parse_pair('512,512') == (512, 512) and slide.parse_pair(' 96 , 128 ') == (96, 128) and slide.parse_pair('64') == (64, 64)
    assert slide.parse_pair('') is None and not slide.is_on(slide.parse_pair('')) and slide.is_on(slide.parse_pair('64,64'))
    for bad in ('1,2,3', '0,4', '4,-1', 'a,b'):
        with pytest.raises(ValueError):
            slide.parse_pair(bad)


def test_default_flags_leave_sliding_off():
    from segland_amd import eval_base, slide
    args = eval_base.get_parser().parse_args([])
    assert (args.slide_crop, args.slide_stride, args.slide_blend, args.slide_mode, args.slide_batch) == ('', '', 'uniform', 'prob', 0)
    assert slide.driver_geometry(args.slide_crop, args.slide_stride) == (None, None)
    on = eval_base.get_parser().parse_args(['--slide-crop', '64,96', '--slide-stride', '32,40', '--slide-blend', 'tent', '--slide-mode', 'logit', '--slide-batch', '3'])
    assert slide.driver_geometry(on.slide_crop, on.slide_stride) == ((64, 96), (32, 40))
    assert (on.slide_blend, on.slide_mode, on.slide_batch) == ('tent', 'logit', 3)
    with pytest.raises(SystemExit):
        eval_base.get_parser().parse_args(['--slide-blend', 'gauss'])


def test_default_stride_is_two_thirds_of_the_crop():
    from segland_amd import slide
    assert slide.default_stride((512, 512)) == (341, 341) and slide.default_stride((64, 96)) == (42, 64) and slide.default_stride((1, 2)) == (1, 1)
    assert slide.driver_geometry('512,512', '') == ((512, 512), (341, 341))
    assert slide.driver_geometry('64,64', '') == ((64, 64), (42, 42))


def test_driver_crop_must_be_a_multiple_of_32():
    from segland_amd import slide
    for bad in ('48,64', '64,100', '16'):
        with pytest.raises(ValueError, match='multiples of 32'):
            slide.driver_geometry(bad, '')
    for bad in ('65,32', '0,8', '32,65'):
        with pytest.raises(ValueError):
            slide.driver_geometry('64,64', bad)
    assert slide.window_grid(40, 16, 8)[0] == 16                   # the library functions take any size
