"""Sliding-window inference fused in one kernel (sl_slide_fuse -> ops.slide_fuse -> segland_amd/slide.py -> eval_base --slide-*) on the GPU: labels and the fused map
against the torch restatement of tests/slide_reference.py (float32, measured against its own float64 evaluation), exact identities with the single-view kernels and
the one-view TTA fusion, the whole path against the CPU oracle, and the evaluation drivers.  Without the entry point, the op and the module every test here fails."""
import os

import numpy as np
import pytest
import torch

import slide_reference as sr
from eval_common import run_eval, top2_margin
from oracle import formula as fm

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MODES = ('prob', 'logit')
BLENDS = ('uniform', 'tent')
_cache = {}


def case_logits(name):
    """(K, size, crop, stride, CPU float32 window logits) of a kernel-level case; built once."""
    if ('logits', name) not in _cache:
        K, size, crop, stride, (h, w), (ys, xs) = sr.CASES[name]
        assert sr.grid(size[0], crop[0], stride[0])[1] == ys and sr.grid(size[1], crop[1], stride[1])[1] == xs
        _cache['logits', name] = (K, size, crop, stride, fm.sym('slide/%s' % name, (sr.BATCH * len(ys) * len(xs), K, h, w), 3.0))
    return _cache['logits', name]


def reference(name, mode, blend, dtype):
    """(labels, fused) of tests/slide_reference.py on the CPU in `dtype`; computed once per (case, mode, blend, dtype) and never modified."""
    key = ('ref', name, mode, blend, dtype)
    if key not in _cache:
        K, size, crop, stride, logits = case_logits(name)
        _cache[key] = sr.fuse(logits.to(dtype), sr.BATCH, size, crop, stride, mode, blend)
    return _cache[key]


def kernel(name, mode, blend, want_map=True):
    from segland_amd import ops
    K, size, crop, stride, logits = case_logits(name)
    return ops.slide_fuse(logits.to(DEV), sr.BATCH, size, crop, stride, mode=mode, blend=blend, want_map=want_map)


@pytest.mark.parametrize('blend', BLENDS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(sr.CASES))
def test_labels_vs_torch_reference(hip, name, mode, blend):
    """Labels equal the float32 reference's argmax wherever its top-2 margin is >= 1e-5; at most 0.5 % of a case's pixels may lie below that margin.  In cases a, b, e and f
    the reference and the kernel predict each of the K classes.  Measured on the MI355X: 0 differing pixels in every case, mode and blend, also among the left-out ones;
    left-out shares (prob uniform / prob tent; 0 in mode logit throughout): a 0 / 0.038 %, b 0.007 / 0.007 %, c 0.114 / 0.038 %, d 0 / 0, e 0 / 0, f 0.056 / 0 %."""
    K, size, crop, stride, _ = case_logits(name)
    ref_labels, ref_fused = reference(name, mode, blend, torch.float32)
    labels, _ = kernel(name, mode, blend)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (sr.BATCH,) + tuple(size)
    labels = labels.cpu().long()
    keep = top2_margin(ref_fused) >= 1e-5
    out_share = 1.0 - float(keep.float().mean())
    differ = int((labels != ref_labels)[keep].sum())
    print('slide case %s mode %s blend %s: %d pixels, %.3f %% below the 1e-5 margin, %d labels differ outside it, %d anywhere' % (
        name, mode, blend, keep.numel(), 100 * out_share, differ, int((labels != ref_labels).sum())))
    assert out_share <= 0.005
    assert differ == 0
    if name in 'abef':
        assert sorted(ref_labels.unique().tolist()) == list(range(K))
        assert sorted(labels.unique().tolist()) == list(range(K))


@pytest.mark.parametrize('blend', BLENDS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(sr.CASES))
def test_fused_map_vs_float64(hip, name, mode, blend):
    """Max abs error of the kernel's map against the float64 evaluation <= max(4 x the float32 torch reference's own error, 2e-6 x max |fused|): the bound of the TTA tests,
    which a weighted mean keeps.  No label of the kernel differs from the float64 labels outside the 1e-5 margin either.  Measured on the MI355X, kernel / float32 torch,
    uniform then tent.  prob: a 2.54e-7 / 2.54e-7 both; b 3.34e-7 / 3.34e-7 both; c 7.05e-8 / 5.97e-8, 7.18e-8 / 8.28e-8; d 3.32e-8 / 3.32e-8 both; e 1.22e-7 / 1.22e-7
    both; f 1.12e-7 / 1.12e-7, 1.50e-7 / 1.50e-7.  logit: a 1.62e-6 / 1.62e-6 both; b 1.77e-6 / 1.71e-6, 1.83e-6 / 1.71e-6; c 5.72e-7 / 5.71e-7, 6.82e-7 / 5.86e-7;
    d 2.38e-7 / 1.99e-7 both; e 5.47e-7 / 5.40e-7, 5.47e-7 / 5.50e-7; f 5.25e-7 / 5.56e-7, 4.51e-7 / 4.77e-7.  Every kernel error is below the floor of its case
    (5.1e-7 to 1.6e-6 in prob, 5.8e-6 to 6.0e-6 in logit)."""
    _, ref32 = reference(name, mode, blend, torch.float32)
    labels64, ref64 = reference(name, mode, blend, torch.float64)
    labels, fused = kernel(name, mode, blend)
    assert fused.dtype == torch.float32 and fused.shape == ref32.shape
    e_kernel = float((fused.cpu().double() - ref64).abs().max())
    e_torch = float((ref32.double() - ref64).abs().max())
    floor = 2e-6 * float(ref64.abs().max())
    print('slide case %s mode %s blend %s: kernel error %.3g, float32 torch error %.3g, floor %.3g' % (name, mode, blend, e_kernel, e_torch, floor))
    assert e_kernel <= max(4 * e_torch, floor)
    assert int((labels.cpu().long() != labels64)[top2_margin(ref64) >= 1e-5].sum()) == 0


@pytest.mark.parametrize('K', [8, 33])
def test_one_window_is_the_single_view_pipeline(hip, K):
    """A crop at least the scene's size gives one window of the scene's own side: uniform + logit is sl_upsample_argmax / sl_upsample_logits bit for bit."""
    from segland_amd import ops
    l = fm.sym('slide/ident/%d' % K, (2, K, 9, 7), 3.0).to(DEV)
    size = (40, 33)
    for crop, stride in (((40, 33), (40, 33)), ((64, 48), (64, 1)), ((41, 33), (7, 33))):
        labels, fused = ops.slide_fuse(l, 2, size, crop, stride, mode='logit', blend='uniform', want_map=True)
        assert torch.equal(labels, ops.upsample_argmax(l, size)), (crop, stride)
        assert torch.equal(fused, ops.upsample_logits(l, size)), (crop, stride)


@pytest.mark.parametrize('mode', MODES)
def test_disjoint_windows_are_one_view_tta(hip, mode):
    """Scene 32x24 with crop = stride = 16x12: every pixel has exactly one window, and each window's block of the map and of the labels is the one-view TTA fusion of that
    window at the crop size, bit for bit."""
    from segland_amd import ops
    K, B = 12, 2
    l = fm.sym('slide/disjoint', (B * 2 * 2, K, 5, 4), 3.0).to(DEV)
    labels, fused = ops.slide_fuse(l, B, (32, 24), (16, 12), (16, 12), mode=mode, blend='uniform', want_map=True)
    for b in range(B):
        for iy in range(2):
            for ix in range(2):
                n = (b * 2 + iy) * 2 + ix
                lab1, map1 = ops.tta_fuse([(l[n:n + 1], 0, 1.0)], (16, 12), mode=mode, want_map=True)
                assert torch.equal(fused[b, :, iy * 16:(iy + 1) * 16, ix * 12:(ix + 1) * 12], map1[0]), (b, iy, ix)
                assert torch.equal(labels[b, iy * 16:(iy + 1) * 16, ix * 12:(ix + 1) * 12], lab1[0]), (b, iy, ix)


@pytest.mark.parametrize('blend', BLENDS)
@pytest.mark.parametrize('mode', MODES)
def test_zero_logits(hip, mode, blend):
    """All-zero logits with K = 8 on case a's geometry: exactly 1/8 (prob) or 0 (logit) everywhere -- integer weights and a power-of-two K leave no rounding -- and label 0."""
    from segland_amd import ops
    K, size, crop, stride, logits = case_logits('a')
    assert K == 8
    labels, fused = ops.slide_fuse(torch.zeros_like(logits).to(DEV), sr.BATCH, size, crop, stride, mode=mode, blend=blend, want_map=True)
    assert int(labels.max()) == 0
    assert torch.equal(fused, torch.full_like(fused, 0.125 if mode == 'prob' else 0.0))


@pytest.mark.parametrize('blend', BLENDS)
@pytest.mark.parametrize('mode', MODES)
def test_two_runs_give_the_same_bits(hip, mode, blend):
    l1, f1 = kernel('b', mode, blend)
    l2, f2 = kernel('b', mode, blend)
    assert torch.equal(l1, l2) and torch.equal(f1, f2)


@pytest.mark.parametrize('blend', BLENDS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['b', 'c', 'f'])
def test_without_the_map(hip, name, mode, blend):
    labels_map, fused = kernel(name, mode, blend, want_map=True)
    labels, none = kernel(name, mode, blend, want_map=False)
    assert none is None and fused is not None
    assert torch.equal(labels, labels_map)


def test_op_refuses(hip):
    from segland_amd import ops
    size, crop, stride = (40, 33), (16, 12), (8, 5)                 # 4 x 6 windows per scene
    a = torch.zeros(2 * 24, 8, 5, 4, device=DEV)
    ops.slide_fuse(a, 2, size, crop, stride)
    for bad in (a[:47], a[:24], torch.zeros(49, 8, 5, 4, device=DEV), a.double(), a.permute(0, 1, 3, 2), a.cpu(), a[0]):
        with pytest.raises(RuntimeError):
            ops.slide_fuse(bad, 2, size, crop, stride)
    for bad_stride in ((0, 5), (8, 0), (17, 5), (8, 13), (-1, 5)):
        with pytest.raises(RuntimeError):
            ops.slide_fuse(a, 2, size, crop, bad_stride)
    with pytest.raises(RuntimeError):
        ops.slide_fuse(a, 2, size, crop, stride, mode='mean')
    with pytest.raises(RuntimeError):
        ops.slide_fuse(a, 2, size, crop, stride, blend='gauss')
    with pytest.raises(RuntimeError):
        ops.slide_fuse(torch.zeros(2 * 24, 34, 5, 4, device=DEV), 2, size, crop, stride)


def whole_path_sides():
    """The HIP model and the CPU oracle with the same formula weights, the image, and the oracle's window logits and whole-image logits; built once for both blends."""
    if 'whole' not in _cache:
        from oracle import pop_oracle as po
        from segland_amd.networks.pspnet_pop import GFSS_Model
        img = fm.formula_image(2, 136, 200, 'slide/model/img')
        m = GFSS_Model(n_base=7, backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=torch.float32)
        fm.load_formula_weights(m)
        m = m.to(DEV).eval()
        o = fm.load_formula_weights(po.PopOracle(n_base=7, criterion=po.OrthLossOracle(255), backbone='resnet50', dilated=True, os=8)).eval()
        (ch, ys), (cw, xs) = sr.grid(136, 96, 40), sr.grid(200, 128, 72)
        assert (ch, ys, cw, xs) == (96, [0, 40], 128, [0, 72])
        with torch.no_grad():
            win = torch.stack([img[b, :, y:y + ch, x:x + cw] for b in range(2) for y in ys for x in xs])
            _cache['whole'] = (m, img, o(win).float().contiguous(), o(img).float().contiguous())
    return _cache['whole']


@pytest.mark.parametrize('blend', BLENDS)
def test_whole_path_vs_cpu_oracle(hip, blend):
    """slide.predict over the HIP model (fp32 mode, 136x200 scenes, crop 96x128, stride 40x72: four windows per image, fused as logits) against the same composition of
    the CPU oracle's forwards: the map within 2e-3 of the oracle map's scale (the project's bound for eval logits; a weighted mean keeps it), labels equal wherever the
    oracle's top-2 margin is >= 4e-3 x scale, with at most 10 % of the pixels below that margin.  The oracle's fused labels differ from its own whole-image labels on more
    than 2 % of the pixels, so a path that ignored the windows cannot pass.  Oracle alone (CPU): scale 1225; 7.71 % (uniform) and 7.30 % (tent) of the pixels below the
    margin; 6.02 % and 5.50 % of the labels moved.  Measured on the MI355X: the same scale and shares, map error 4.16e-6 (uniform) and 4.34e-6 (tent) of scale, no label
    differs outside the margin."""
    import torch.nn.functional as F
    from segland_amd import slide
    m, img, win_logits, whole_logits = whole_path_sides()
    size, crop, stride = (136, 200), (96, 128), (40, 72)
    pred, fused = slide.predict(m, img.to(DEV), crop, stride, mode='logit', blend=blend, want_map=True)
    ref_labels, ref_fused = sr.fuse(win_logits, 2, size, crop, stride, 'logit', blend)
    whole_labels = F.interpolate(whole_logits, size=size, mode='bilinear', align_corners=True).argmax(dim=1)
    scale = float(ref_fused.abs().max())
    assert tuple(fused.shape) == tuple(ref_fused.shape) and tuple(pred.shape) == (2,) + size
    err = float((fused.cpu() - ref_fused).abs().max()) / scale
    keep = top2_margin(ref_fused) >= 4e-3 * scale
    out_share = 1.0 - float(keep.float().mean())
    differ = int((pred.cpu().long() != ref_labels)[keep].sum())
    moved = float((ref_labels != whole_labels).float().mean())
    print('slide whole path, blend %s: scale %.4g, map error %.3g of scale, %.2f %% of pixels below the margin, %d labels differ outside it, the windows move %.2f %% of the '
          'oracle labels' % (blend, scale, err, 100 * out_share, differ, 100 * moved))
    assert err <= 2e-3
    assert out_share <= 0.10
    assert differ == 0
    assert moved > 0.02                     # a property of the oracle alone: the windows matter, so ignoring them cannot pass the label gate


def test_eval_driver_with_sliding(hip, tmp_path):
    """eval_base --slide-crop 64,64 scores the same pixels as the plain run; with --save-prob the .mat holds the fused map, its argmax is the PNG, and fusemat takes it."""
    import scipy.io
    from PIL import Image
    from segland_amd import fusemat
    plain = run_eval(tmp_path / 'plain', [])
    slid = run_eval(tmp_path / 'slide', ['--slide-crop', '64,64'])
    assert slid.shape == plain.shape and slid.sum() == plain.sum() > 0
    dump = run_eval(tmp_path / 'dump', ['--slide-crop', '64,64', '--save-prob'])
    assert np.array_equal(dump, slid)
    prob = str(tmp_path / 'dump' / 'prob_123')
    out = scipy.io.loadmat(os.path.join(prob, '0.mat'))['outputs']
    assert out.shape == (1, 8, 128, 128) and out.dtype == np.float32        # the base model's logit channels: background + 7 base classes
    assert abs(float(out[0].sum(0).mean()) - 1.0) < 1e-5                    # mode prob: a probability map
    png = np.array(Image.open(os.path.join(prob + '_png', '0.png')))
    assert np.array_equal(out[0].argmax(0), png)
    res = fusemat.fuse([prob], str(tmp_path / 'fused'), size=(128, 128))
    assert np.array_equal(res['0.mat'], png)
    log = ''.join(open(os.path.join(str(tmp_path / 'slide'), f)).read() for f in os.listdir(str(tmp_path / 'slide')) if f.endswith('.log'))
    assert 'sliding-window inference: 9 windows per tile' in log and 'crop 64x64, stride 42x42, blend uniform, mode prob' in log


def test_eval_driver_default_flags_do_not_call_the_op(hip, tmp_path, monkeypatch):
    from segland_amd import ops

    def refuse(*a, **k):
        raise AssertionError('ops.slide_fuse called')
    monkeypatch.setattr(ops, 'slide_fuse', refuse)
    cm = run_eval(tmp_path / 'plain', [])
    assert cm.sum() > 0
    with pytest.raises(AssertionError, match='ops.slide_fuse called'):
        run_eval(tmp_path / 'on', ['--slide-crop', '64,64'])


def test_eval_driver_refuses_sliding_with_tta_and_unaligned_crops(hip, tmp_path):
    with pytest.raises(ValueError, match='tta'):
        run_eval(tmp_path / 'both', ['--slide-crop', '64,64', '--tta-flip', 'True'])
    with pytest.raises(ValueError, match='multiples of 32'):
        run_eval(tmp_path / 'odd', ['--slide-crop', '48,64'])


def test_eval_ft_driver_with_sliding(hip, tmp_path):
    """The eval_ft call (long-side square: the image grid for a square tile) with windows forwarded three at a time: same pixels scored as without sliding."""
    from segland_amd.networks.pspnet_pop import GFSS_Model
    torch.manual_seed(0)
    m = GFSS_Model(n_base=7, backbone='resnet50', dilated=True, os=8, n_novel=4, is_ft=True, pretrained_model=None)
    torch.save({'module.' + k: v for k, v in m.state_dict().items()}, str(tmp_path / 'novel_123.pth'), _use_new_zipfile_serialization=False)
    from segland_amd import eval_base
    argv = ['--model', 'pspnet_pop', '--backbone', 'resnet50', '--dataset', 'synthetic', '--base-size', '128,128', '--fp16', '--restore-from', str(tmp_path / 'novel.pth'),
            '--random-seed', '123']
    cms = []
    for name, extra in (('plain', []), ('slide', ['--slide-crop', '64,64', '--slide-batch', '3'])):
        eval_base.main(argv + ['--save-path', str(tmp_path / name)] + extra, ft=True)
        cms.append(np.load(str(tmp_path / name / 'cmatrix_123.npy')))
    assert cms[0].shape == (12, 12) and cms[1].sum() == cms[0].sum() > 0
