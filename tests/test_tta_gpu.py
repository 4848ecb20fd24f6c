"""Multi-scale + flip test-time augmentation fused in one kernel (sl_tta_fuse -> ops.tta_fuse -> segland_amd/tta.py -> eval_base --tta-*) on the GPU: labels and the
fused map against the torch restatement of tests/tta_reference.py (float32, measured against its own float64 evaluation), exact identities with the single-view kernels
and under flips, the whole path against the CPU oracle, and the evaluation drivers.  Without the entry point, the op and the module every test here fails."""
import os

import numpy as np
import pytest
import torch

import tta_reference as tr
from eval_common import run_eval, top2_margin
from oracle import formula as fm

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MODES = ('prob', 'logit')
_cache = {}


def case_views(name):
    """(K, size, CPU float32 views) of a kernel-level case; built once."""
    if ('views', name) not in _cache:
        K, size, specs = tr.CASES[name]
        _cache['views', name] = (K, size, [(fm.sym('tta/%s/%d' % (name, i), (2, K, h, w), 3.0), f, wt) for i, (h, w, f, wt) in enumerate(specs)])
    return _cache['views', name]


def reference(name, mode, dtype):
    """(labels, fused) of tests/tta_reference.py on the CPU in `dtype`; computed once per (case, mode, dtype) and never modified."""
    key = ('ref', name, mode, dtype)
    if key not in _cache:
        K, size, views = case_views(name)
        _cache[key] = tr.fuse([(l.to(dtype), f, wt) for l, f, wt in views], size, mode)
    return _cache[key]


def on_gpu(views):
    return [(l.to(DEV), f, wt) for l, f, wt in views]


def kernel(name, mode, want_map=True):
    from segland_amd import ops
    K, size, views = case_views(name)
    return ops.tta_fuse(on_gpu(views), size, mode=mode, want_map=want_map)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(tr.CASES))
def test_labels_vs_torch_reference(hip, name, mode):
    """Labels equal the float32 reference's argmax wherever its top-2 margin is >= 1e-5; at most 0.5 % of a case's pixels may lie below that margin.  Every case but the
    one-pixel one predicts each of its K classes.  Measured on the MI355X: 0 differing pixels in every case and mode, also among the left-out ones; left-out share at most
    0.114 % (case c, prob)."""
    K, size, _ = case_views(name)
    ref_labels, ref_fused = reference(name, mode, torch.float32)
    labels, _ = kernel(name, mode)
    labels = labels.cpu().long()
    assert labels.shape == ref_labels.shape and labels.dtype == torch.int64
    keep = top2_margin(ref_fused) >= 1e-5
    out_share = 1.0 - float(keep.float().mean())
    differ = int((labels != ref_labels)[keep].sum())
    print('tta case %s mode %s: %d pixels, %.3f %% below the 1e-5 margin, %d labels differ outside it, %d anywhere' % (
        name, mode, keep.numel(), 100 * out_share, differ, int((labels != ref_labels).sum())))
    assert out_share <= 0.005
    assert differ == 0
    if name != 'd':
        assert sorted(ref_labels.unique().tolist()) == list(range(K))
        assert sorted(labels.unique().tolist()) == list(range(K))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(tr.CASES))
def test_fused_map_vs_float64(hip, name, mode):
    """Max abs error of the kernel's map against the float64 evaluation <= max(4 x the float32 torch reference's own error, 2e-6 x max |fused|): the floor is the
    project's bound for upsample_logits, the factor covers the kernel's own expf and order of operations.  Measured on the MI355X (kernel / torch): prob a 3.51e-7 / 3.20e-7,
    b 3.32e-7 / 3.17e-7, c 1.33e-7 / 1.33e-7, d 2.07e-8 / 2.07e-8, e 4.59e-7 / 4.89e-7; logit a 1.12e-6, b 1.93e-6, c 1.20e-6, d 5.96e-8, e 2.52e-6 on both sides."""
    _, ref32 = reference(name, mode, torch.float32)
    _, ref64 = reference(name, mode, torch.float64)
    _, fused = kernel(name, mode)
    assert fused.dtype == torch.float32 and fused.shape == ref32.shape
    e_kernel = float((fused.cpu().double() - ref64).abs().max())
    e_torch = float((ref32.double() - ref64).abs().max())
    floor = 2e-6 * float(ref64.abs().max())
    print('tta case %s mode %s: kernel error %.3g, float32 torch error %.3g, floor %.3g' % (name, mode, e_kernel, e_torch, floor))
    assert e_kernel <= max(4 * e_torch, floor)


@pytest.mark.parametrize('K', [8, 33])
def test_identities(hip, K):
    """One plain view in mode logit is the single-view pipeline bit for bit; a flipped view alone is the flipped output of the plain one, labels and map, in both modes."""
    from segland_amd import ops
    l = fm.sym('tta/ident/%d' % K, (2, K, 9, 7), 3.0).to(DEV)
    size = (40, 33)
    labels, fused = ops.tta_fuse([(l, 0, 1.0)], size, mode='logit', want_map=True)
    assert torch.equal(labels, ops.upsample_argmax(l, size))
    assert torch.equal(fused, ops.upsample_logits(l, size))
    for mode in MODES:
        labels0, fused0 = ops.tta_fuse([(l, 0, 1.0)], size, mode=mode, want_map=True)
        for f in (1, 2, 3):
            labels_f, fused_f = ops.tta_fuse([(l, f, 1.0)], size, mode=mode, want_map=True)
            dims = tr.flip_dims(f)
            assert torch.equal(labels_f, torch.flip(labels0, dims)), (mode, f)
            assert torch.equal(fused_f, torch.flip(fused0, dims)), (mode, f)
    z = torch.zeros_like(l)
    for mode in MODES:
        labels, fused = ops.tta_fuse([(z, 0, 1.0), (z, 1, 1.0)], size, mode=mode, want_map=True)
        assert int(labels.max()) == 0
        assert torch.equal(fused, torch.full_like(fused, 1.0 / K if mode == 'prob' else 0.0))


@pytest.mark.parametrize('mode', MODES)
def test_two_runs_give_the_same_bits(hip, mode):
    l1, f1 = kernel('b', mode)
    l2, f2 = kernel('b', mode)
    assert torch.equal(l1, l2) and torch.equal(f1, f2)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['b', 'c'])
def test_without_the_map(hip, name, mode):
    labels_map, fused = kernel(name, mode, want_map=True)
    labels, none = kernel(name, mode, want_map=False)
    assert none is None and fused is not None
    assert torch.equal(labels, labels_map)


def test_op_refuses_mismatched_views(hip):
    from segland_amd import ops
    a = torch.zeros(2, 8, 9, 7, device=DEV)
    for bad in (torch.zeros(2, 9, 9, 7, device=DEV), torch.zeros(1, 8, 9, 7, device=DEV), a.double(), a.permute(0, 1, 3, 2), torch.zeros(2, 8, 9, 7)):
        with pytest.raises(RuntimeError):
            ops.tta_fuse([(a, 0, 1.0), (bad, 1, 1.0)], (40, 33))
    with pytest.raises(RuntimeError):
        ops.tta_fuse([(a, 0, 1.0)], (40, 33), mode='mean')
    with pytest.raises(RuntimeError):
        ops.tta_fuse([(a, 4, 1.0)], (40, 33))
    with pytest.raises(RuntimeError):
        ops.tta_fuse([(a, 0, 0.0)], (40, 33))


def test_whole_path_vs_cpu_oracle(hip):
    """tta.predict over the HIP model (fp32 mode, two scales, each plain and mirrored, fused as logits) against the same composition of the CPU oracle's forwards:
    the map within 2e-3 of the oracle map's scale (the bound of test_configs_vs_same_box_oracle for eval logits at these image sizes; a weighted mean keeps it), labels
    equal wherever the oracle's top-2 margin is >= 4e-3 x scale, with at most 10 % of the pixels below that margin.  The oracle's fused labels differ from its single-view
    labels on about 11.6 % of the pixels, so a pipeline that ignored the extra views cannot pass.  Measured on the MI355X: scale 889.1, map error 3.09e-6 of scale,
    6.94 % of the pixels below the margin, no label differs outside it, the views move 11.58 % of the oracle's labels."""
    import torch.nn.functional as F
    from oracle import pop_oracle as po
    from segland_amd import tta
    from segland_amd.networks.pspnet_pop import GFSS_Model
    img = fm.formula_image(2, 72, 104, 'tta/model/img')
    m = GFSS_Model(n_base=7, backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=torch.float32)
    fm.load_formula_weights(m)
    m = m.to(DEV).eval()
    o = fm.load_formula_weights(po.PopOracle(n_base=7, criterion=po.OrthLossOracle(255), backbone='resnet50', dilated=True, os=8)).eval()
    size, scales = (72, 104), (1.0, 1.9)
    pred, fused = tta.predict(m, img.to(DEV), size, scales=scales, flip=True, mode='logit', want_map=True, align=8)
    views = []
    with torch.no_grad():
        for s in scales:
            im = img if s == 1.0 else F.interpolate(img, tta.scaled_size(72, 104, s, 8), mode='bilinear', align_corners=False)
            views.append((o(im).float().contiguous(), 0, 1.0))
            views.append((o(im.flip(-1)).float().contiguous(), 1, 1.0))
    assert [tuple(im_hw) for im_hw in tta.view_sizes(72, 104, scales, 8)] == [(72, 104), (136, 200)]
    ref_labels, ref_fused = tr.fuse(views, size, 'logit')
    single_labels, _ = tr.fuse(views[:1], size, 'logit')
    scale = float(ref_fused.abs().max())
    err = float((fused.cpu() - ref_fused).abs().max()) / scale
    keep = top2_margin(ref_fused) >= 4e-3 * scale
    out_share = 1.0 - float(keep.float().mean())
    differ = int((pred.cpu().long() != ref_labels)[keep].sum())
    moved = float((ref_labels != single_labels).float().mean())
    print('tta whole path: scale %.4g, map error %.3g of scale, %.2f %% of pixels below the margin, %d labels differ outside it, the views move %.2f %% of the oracle labels'
          % (scale, err, 100 * out_share, differ, 100 * moved))
    assert tuple(fused.shape) == tuple(ref_fused.shape)
    assert err <= 2e-3
    assert out_share <= 0.10
    assert differ == 0
    assert moved > 0.02                     # a property of the oracle alone (11.6 % on the CPU): the extra views matter, so ignoring them cannot pass the label gate


def test_eval_driver_with_flip(hip, tmp_path):
    """eval_base --tta-flip True scores the same pixels as the plain run; with --save-prob the .mat holds the fused map, its argmax is the PNG, and fusemat takes it."""
    import scipy.io
    from PIL import Image
    from segland_amd import fusemat
    plain = run_eval(tmp_path / 'plain', [])
    flip = run_eval(tmp_path / 'flip', ['--tta-flip', 'True'])
    assert flip.shape == plain.shape and flip.sum() == plain.sum() > 0
    dump = run_eval(tmp_path / 'dump', ['--tta-flip', 'True', '--save-prob'])
    assert np.array_equal(dump, flip)
    prob = str(tmp_path / 'dump' / 'prob_123')
    out = scipy.io.loadmat(os.path.join(prob, '0.mat'))['outputs']
    assert out.shape == (1, 8, 128, 128) and out.dtype == np.float32        # the base model's logit channels: background + 7 base classes
    assert abs(float(out[0].sum(0).mean()) - 1.0) < 1e-5                    # mode prob: a probability map
    png = np.array(Image.open(os.path.join(prob + '_png', '0.png')))
    assert np.array_equal(out[0].argmax(0), png)
    res = fusemat.fuse([prob], str(tmp_path / 'fused'), size=(128, 128))
    assert np.array_equal(res['0.mat'], png)


def test_eval_driver_default_flags_do_not_call_the_op(hip, tmp_path, monkeypatch):
    from segland_amd import ops

    def refuse(*a, **k):
        raise AssertionError('ops.tta_fuse called with the default flags')
    monkeypatch.setattr(ops, 'tta_fuse', refuse)
    cm = run_eval(tmp_path / 'plain', ['--tta-scales', '1.0', '--tta-flip', 'False'])
    assert cm.sum() > 0
    with pytest.raises(AssertionError):
        run_eval(tmp_path / 'on', ['--tta-flip', 'True'])


def test_eval_ft_driver_with_flip(hip, tmp_path):
    """The eval_ft call (long-side square, labels padded with ignore) with the mirrored view: same pixels scored as without it."""
    from segland_amd.networks.pspnet_pop import GFSS_Model
    torch.manual_seed(0)
    m = GFSS_Model(n_base=7, backbone='resnet50', dilated=True, os=8, n_novel=4, is_ft=True, pretrained_model=None)
    torch.save({'module.' + k: v for k, v in m.state_dict().items()}, str(tmp_path / 'novel_123.pth'), _use_new_zipfile_serialization=False)
    from segland_amd import eval_base
    argv = ['--model', 'pspnet_pop', '--backbone', 'resnet50', '--dataset', 'synthetic', '--base-size', '128,128', '--fp16', '--restore-from', str(tmp_path / 'novel.pth'),
            '--random-seed', '123']
    cms = []
    for name, extra in (('plain', []), ('flip', ['--tta-flip', 'True'])):
        eval_base.main(argv + ['--save-path', str(tmp_path / name)] + extra, ft=True)
        cms.append(np.load(str(tmp_path / name / 'cmatrix_123.npy')))
    assert cms[0].shape == (12, 12) and cms[1].sum() == cms[0].sum() > 0
