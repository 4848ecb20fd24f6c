"""CPU-only part of the boundary scores (sl_boundary_counts -> ops.boundary_counts -> eval_base --boundary-width): the numpy contract of tests/boundary_reference.py
against the published per-class erosion form, the properties that tie its outputs together, the host helper, and the ABI's refusals, which return before any launch.
The ABI and parser tests fail without the entry point and the flag."""
import ctypes as C
import os

import numpy as np
import pytest

import boundary_reference as br


@pytest.fixture(scope='module')
def lib():
    from segland_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def blobs(rng, B, H, W, K):
    """Blobby label maps with every pixel a class: pred is target with noise on the class scores."""
    z = rng.random((B, K, H, W))
    for _ in range(8):                                               # a few 3x3 box means
        z = sum(np.roll(np.roll(z, dy, 2), dx, 3) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    z /= z.max()
    return (z + 0.02 * rng.random(z.shape)).argmax(1).astype(np.uint8), z.argmax(1).astype(np.int64)


@pytest.mark.parametrize('shape', [(2, 37, 53, 5, 1), (1, 70, 66, 12, 3), (1, 67, 40, 33, 32), (2, 16, 16, 3, 5)])
def test_contract_equals_per_class_erosion(shape):
    """Without ignored pixels the contract's counts are those of mask_to_boundary per class: 1 px of zeros around the mask, d erosions with the 3x3 element."""
    B, H, W, K, d = shape
    pred, target = blobs(np.random.default_rng(H * W + d), B, H, W, K)
    counts, band_cm, _, _ = br.contract_counts(pred, target, K, 255, d)
    assert np.array_equal(counts, br.erosion_counts(pred, target, K, d))
    assert counts[1].sum() > 0 and np.array_equal(band_cm.sum(1), counts[1])


def test_voronoi_cases_without_ignore_equal_erosion_too():
    for name in ('ragged', 'small', 'row129'):
        (B, H, W, K, d) = br.CASES[name][0]
        pred, target = br.case_maps(name)
        assert np.array_equal(br.case_reference(name)[0], br.erosion_counts(pred, target, K, d)), name


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_properties_with_ignore_regions(seed):
    """band_cm's rows sum to the ground-truth band counts when every pred is a class; the intersection is within both bands; the trimap matrix is within the full one."""
    rng = np.random.default_rng(seed)
    B, H, W, K, d = 2, 40, 57, 6, 1 + seed
    pred, target = blobs(rng, B, H, W, K)
    target[0, 5:20, 10:30] = 255
    target[1, :, :4] = 255
    target.reshape(-1)[rng.integers(0, target.size, 8)] = -1
    counts, band_cm, _, _ = br.contract_counts(pred, target, K, 255, d)
    assert np.array_equal(band_cm.sum(1), counts[1])
    assert (counts[0] <= np.minimum(counts[1], counts[2])).all() and counts[0].sum() > 0
    cm = br.confusion(pred, target, K, 255)
    assert (band_cm <= cm).all() and 0 < band_cm.sum() < cm.sum()
    pred.reshape(-1)[rng.integers(0, pred.size, 40)] = K + 1          # pred >= K: such pixels leave band_cm's rows but stay in counts[1]
    counts2, band_cm2, _, _ = br.contract_counts(pred, target, K, 255, d)
    assert (band_cm2.sum(1) <= counts2[1]).all() and band_cm2.sum() < counts2[1].sum()


def test_every_case_meets_the_cover_condition():
    """The label maps of the GPU cases: both bands of the reference cover part of the map, never all of it, except in the case meant to saturate (all of it)."""
    for name, (shape, _, saturating, _) in br.CASES.items():
        _, _, g, p = br.case_reference(name)
        assert (g == 1.0 and p == 1.0) if saturating else (0.0 < g < 1.0 and 0.0 < p < 1.0), (name, g, p)


def test_boundary_iou_from_counts():
    from segland_amd.eval_base import boundary_iou_from_counts
    #                 inter              ground-truth band     prediction band           classes 0..2 base (n_base = 2), 3..5 novel; classes 1 and 4 absent
    counts = np.array([[2, 0, 3, 5, 0, 0], [4, 0, 3, 10, 0, 6], [6, 0, 3, 5, 0, 2]], np.int64)
    iou, base, novel, total = boundary_iou_from_counts(counts, 2)
    want = np.array([2 / 8, np.nan, 1.0, 5 / 10, np.nan, 0.0])
    assert np.array_equal(np.isnan(iou), np.isnan(want)) and np.allclose(iou[~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=1e-15)
    assert base == pytest.approx((0.25 + 1.0) / 2) and novel == pytest.approx((0.5 + 0.0) / 2) and total == pytest.approx((0.25 + 1.0 + 0.5 + 0.0) / 4)
    iou, base, novel, total = boundary_iou_from_counts(counts[:, :3], 2)            # no novel class at all
    assert base == total == pytest.approx(0.625) and np.isnan(novel)
    iou, base, novel, total = boundary_iou_from_counts(np.zeros((3, 4), np.int64), 1)
    assert np.isnan(iou).all() and np.isnan(base) and np.isnan(novel) and np.isnan(total)


def test_symbol_is_exported_and_declared(lib):
    from segland_amd import _lib
    decl = _lib.declared_functions()
    assert 'sl_boundary_counts' in decl and hasattr(lib, 'sl_boundary_counts')
    restype, argtypes = decl['sl_boundary_counts']
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3


def test_bad_arguments_are_refused_without_launch(lib):
    dummy = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string()
    ok = dict(pred=dummy, target=dummy, B=1, H=8, W=8, K=5, ign=255, d=3, counts=dummy, band_cm=dummy)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sl_boundary_counts(a['pred'], a['target'], a['B'], a['H'], a['W'], a['K'], a['ign'], a['d'], a['counts'], a['band_cm'], None)
    for name in ('pred', 'target', 'counts', 'band_cm'):
        assert call(**{name: None}) == -1 and b'NULL' in err(), name
    for name in ('B', 'H', 'W'):
        for v in (0, -3):
            assert call(**{name: v}) == -1 and b'at least 1' in err(), (name, v)
    for K in (0, 65, -1):
        assert call(K=K) == -1 and b'classes outside [1, 64]' in err(), K
    for d in (0, 33, -2):
        assert call(d=d) == -1 and b'outside [1, 32]' in err(), d


def test_op_refuses_cpu_tensors():
    import torch
    from segland_amd import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.boundary_counts(torch.zeros((1, 8, 8), dtype=torch.uint8), torch.zeros((1, 8, 8), dtype=torch.int64), 5, 255, 3)
    with pytest.raises(ValueError, match='one shape'):
        ops.boundary_counts(torch.zeros((1, 8, 8), dtype=torch.uint8), torch.zeros((1, 8, 9), dtype=torch.int64), 5, 255, 3)


def test_parser_flag(capsys):
    from segland_amd import eval_base
    assert eval_base.get_parser().parse_args([]).boundary_width == 0
    assert eval_base.get_parser().parse_args(['--boundary-width', '32']).boundary_width == 32
    for bad in ('33', '-1', 'wide'):
        with pytest.raises(SystemExit):
            eval_base.get_parser().parse_args(['--boundary-width', bad])
        assert '--boundary-width' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        eval_base.get_parser().parse_args(['--boundary-width', '33'])
    assert 'outside 0..32' in capsys.readouterr().err
