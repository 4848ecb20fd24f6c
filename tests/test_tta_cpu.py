"""Multi-scale + flip test-time augmentation, CPU side: sl_tta_fuse is declared and exported and refuses every bad argument before any launch (a dummy pointer, no
device), the scale list and the view sizes of segland_amd/tta.py, and the evaluation parser leaves the augmentation off by default."""
import ctypes as C
import math
import os

import pytest


@pytest.fixture(scope='module')
def lib():
    from segland_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_entry_point_is_declared_and_exported(lib):
    from segland_amd import _lib
    decl = _lib.declared_functions()
    assert 'sl_tta_fuse' in decl and len(decl['sl_tta_fuse'][1]) == 9
    assert hasattr(lib, 'sl_tta_fuse')
    header = open(_lib.HEADER).read()
    assert '#define SL_TTA_MAX_VIEWS 16' in header and _lib.SL_TTA_MAX_VIEWS == 16
    # the ctypes mirror has the layout of the C struct: int n, 16 pointers (8-aligned), 3 x 16 ints, 16 floats
    assert C.sizeof(_lib.SlTtaViews) == 8 + 16 * 8 + 4 * 16 * 4 and _lib.SlTtaViews.logits.offset == 8


def good_views(n=2):
    from segland_amd import _lib
    v = _lib.SlTtaViews()
    v.n = n
    for i in range(n):
        v.logits[i], v.h[i], v.w[i], v.flip[i], v.weight[i] = 16, 9, 7, i & 3, 1.0
    return v


def test_bad_arguments_are_refused_before_any_launch(lib):
    d = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string().decode()

    def call(v=None, B=2, K=8, H=40, W=33, mode=0, labels=d, views_ptr=True):
        v = good_views() if v is None else v
        return lib.sl_tta_fuse(C.byref(v) if views_ptr else None, B, K, H, W, mode, labels, None, None)

    assert call(views_ptr=False) == -1 and 'tta_fuse' in err()
    assert call(labels=None) == -1 and 'tta_fuse' in err()
    assert call(K=34) == -1 and '34 logit channels' in err() and 'at most 33' in err()
    assert call(K=0) == -1 and 'tta_fuse' in err()
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(mode=2), dict(mode=-1)):
        assert call(**kw) == -1 and 'tta_fuse' in err(), kw
    for n in (0, -1, 17):
        v = good_views(); v.n = n
        assert call(v) == -1 and 'views' in err(), n
    for field, value in (('logits', None), ('h', 0), ('w', 0), ('flip', 4), ('flip', -1), ('weight', 0.0), ('weight', -1.0), ('weight', math.inf), ('weight', math.nan)):
        v = good_views()
        getattr(v, field)[1] = value
        assert call(v) == -1 and 'view 1' in err(), (field, value)


def test_parse_scales():
    from segland_amd import tta
    assert tta.parse_scales('0.75,1.0,1.25') == (0.75, 1.0, 1.25)
    assert tta.parse_scales('1.0') == (1.0,)
    for bad in ('', ' , ', '0', '1.0,-0.5', 'inf', '1.0,nan'):
        with pytest.raises(ValueError):
            tta.parse_scales(bad)


def test_scaled_size():
    from segland_amd import tta
    assert tta.scaled_size(72, 104, 1.9, 8) == (136, 200)
    assert tta.scaled_size(128, 128, 0.75, 32) == (96, 96)
    assert tta.scaled_size(73, 101, 1.0, 32) == (73, 101)          # scale 1.0: the image as it is, aligned or not
    assert tta.scaled_size(40, 40, 0.1, 32) == (32, 32)            # never below one alignment unit


def test_more_than_sixteen_views_raise():
    import torch
    from segland_amd import tta
    with pytest.raises(ValueError):
        tta.views(lambda im: im, torch.zeros(1, 3, 8, 8), (1.0,) * 9, True)
    with pytest.raises(ValueError):
        tta.views(lambda im: im, torch.zeros(1, 3, 8, 8), (1.0,) * 17, False)


def test_views_order_and_flags():
    """Per scale the plain view, then the mirrored one; scale 1.0 hands the image through untouched.  A stand-in model (the identity) on the CPU: views() itself is plumbing."""
    import torch
    from segland_amd import tta
    img = torch.arange(2 * 3 * 8 * 16, dtype=torch.float32).reshape(2, 3, 8, 16)
    seen = []
    vs = tta.views(lambda im: (seen.append(im), im)[1], img, (1.0, 2.0), True, align=8)
    assert [(tuple(v[0].shape[-2:]), v[1], v[2]) for v in vs] == [((8, 16), 0, 1.0), ((8, 16), 1, 1.0), ((16, 32), 0, 1.0), ((16, 32), 1, 1.0)]
    assert seen[0] is img and torch.equal(seen[1], img.flip(-1)) and torch.equal(seen[3], seen[2].flip(-1))
    assert all(v[0].dtype == torch.float32 and v[0].is_contiguous() for v in vs)


def test_default_flags_leave_tta_off():
    from segland_amd import eval_base, tta
    args = eval_base.get_parser().parse_args([])
    assert args.tta_scales == '1.0' and args.tta_flip is False and args.tta_mode == 'prob'
    assert not tta.is_on(tta.parse_scales(args.tta_scales), args.tta_flip)
    on = eval_base.get_parser().parse_args(['--tta-scales', '0.75,1.0', '--tta-flip', 'True', '--tta-mode', 'logit'])
    assert on.tta_flip is True and on.tta_mode == 'logit' and tta.is_on(tta.parse_scales(on.tta_scales), on.tta_flip)
    assert tta.is_on((1.0,), True) and tta.is_on((0.5,), False) and tta.is_on((1.0, 1.0), False)
