#!/usr/bin/env python3
"""Generalised few-shot evaluation entry points (counterparts of the reference's eval_base.py / eval_ft.py) on the MI355X HIP path.

    python -m segland_amd.eval_base --model pspnet_pop --backbone resnet50 --dataset synthetic --restore-from best.pth --save-path out
    python -m segland_amd.eval_ft   ... --random-seed 123,234 --restore-from novel.pth      # loads novel_<seed>.pth per seed

One loop serves every mode.  Per batch: the grid the prediction is scored at (label_grid: the label's own, or eval_ft's long-side square; the image's for unlabeled test
tiles, eval_base.py:178-191, where the prediction and the dump are the product) -> predict -> confusion-matrix kernel -> with --save-prob the .mat / TIFF / PNG dump
(dump_maps); mIoU over base / novel / all classes from the accumulated matrix exactly as eval_base.py:193-199.  select_predictor picks `predict` once from the flags:
plain (the default): logits (eval-mode forward, folded BN) -> upsample(align_corners=True) + argmax in ONE kernel (the H x W logits of eval_base.py:168 are never
  written); with --save-prob the .mat holds the logits upsampled to the tile's own size.  Neither fusion kernel is called.
--tta-scales 0.75,1.0,1.25 --tta-flip True [--tta-mode prob|logit]: test-time augmentation (segland_amd/tta.py).  One forward per view (scale, plain / mirrored), then ONE
  kernel upsamples every view to the scoring grid, takes the softmax (prob) or not (logit), un-flips, averages and takes the argmax.
--slide-crop 512,512 [--slide-stride 341,341] [--slide-blend uniform|tent] [--slide-mode prob|logit] [--slide-batch N]: sliding-window inference (segland_amd/slide.py).
  The tile is cut into overlapping windows of the crop (the size the model was trained at), forwarded N at a time, then ONE kernel upsamples every window's logits to the
  crop, takes the softmax or not, weights them (uniform, or a tent that favours a window's centre), averages the windows over each pixel and takes the argmax.  Refused:
  sliding together with --tta-*, or with a scoring grid that is not the image grid (eval_ft's long-side square of a non-square tile).
--boundary-width D (1..32 pixels; 0 = off, the default): contour scores beside mIoU, whichever predictor made `pred`.  ONE more kernel per batch (sl_boundary_counts) counts
  the Boundary IoU terms and the trimap confusion matrix of the pixels within D of a class border; bcounts_<seed>.npy / band_cmatrix_<seed>.npy and six log lines.
The two fusing modes put their fused map, cut to the tile, into the .mat and state their geometry in one log line at the first batch.
"""
import argparse
import os
import os.path as osp
import warnings

import numpy as np
import torch

from . import dataset as dataset_pkg
from . import networks
from . import ops
from . import slide
from . import tta
from .drivers import batch_to_device, checkpoint_or_none, compute_dtype, resolve, str2bool
from .engine import Engine
from .utils import pyt_utils as my_utils


def get_parser():
    """Flag names and defaults of eval_base.py:36-72 (+ --fp16 selecting bf16 MFMA, as in the training drivers)."""
    p = argparse.ArgumentParser(description='SegLand evaluation on the MI355X HIP path')
    p.add_argument('--dataset', type=str, default='synthetic')
    p.add_argument('--data-dir', type=str, default='')
    p.add_argument('--train-list', type=str, default='')
    p.add_argument('--val-list', type=str, default='')
    p.add_argument('--test-batch-size', type=int, default=1)
    p.add_argument('--model', type=str, default='pspnet_pop')
    p.add_argument('--restore-from', type=str, default='')
    p.add_argument('--backbone', type=str, default='resnet101')
    p.add_argument('--base-size', type=str, default='512,512')
    p.add_argument('--num-workers', type=int, default=0)
    p.add_argument('--save', type=str2bool, default='False')
    p.add_argument('--os', type=int, default=8)
    p.add_argument('--save-path', type=str, default='')
    p.add_argument('--random-seed', type=str, default='123')
    p.add_argument('--fold', type=int, default=0, choices=[0, 1, 2, 3])
    p.add_argument('--shot', type=int, default=1)
    p.add_argument('--fp16', action='store_true')
    p.add_argument('--save-prob', action='store_true', help="dump the upsampled logits of every tile as <save-path>/prob_<seed>/<id>.mat ({'outputs': [1,K,H,W]}, "
                   'eval_base.py:189-190) for segland_amd.fusemat, plus the predicted label map as a palette PNG')
    p.add_argument('--tta-scales', type=str, default='1.0', help="test-time augmentation: image scales of the views, e.g. '0.75,1.0,1.25' (sides rounded to multiples of 32)")
    p.add_argument('--tta-flip', type=str2bool, default='False', help='test-time augmentation: add the horizontally mirrored view of every scale')
    p.add_argument('--tta-mode', type=str, default='prob', choices=['prob', 'logit'], help='the views are fused as softmax probabilities or as upsampled logits (one kernel, '
                   'segland_amd.tta); with --save-prob the .mat holds the fused map')
    p.add_argument('--slide-crop', type=str, default='', help="sliding-window inference: window size 'H,W' (multiples of 32), e.g. '512,512' for 1024x1024 tiles; empty = off")
    p.add_argument('--slide-stride', type=str, default='', help="sliding-window inference: window stride 'H,W', each within [1, crop]; default: two thirds of the crop, rounded down")
    p.add_argument('--slide-blend', type=str, default='uniform', choices=['uniform', 'tent'], help='weights of the overlapping windows: all one, or min(y+1, ch-y) * min(x+1, cw-x)')
    p.add_argument('--slide-mode', type=str, default='prob', choices=['prob', 'logit'], help='the windows are fused as softmax probabilities or as upsampled logits (one kernel, '
                   'segland_amd.slide); with --save-prob the .mat holds the fused map')
    p.add_argument('--slide-batch', type=int, default=0, help='sliding-window inference: windows per forward (0 = all windows of a batch at once)')
    p.add_argument('--boundary-width', type=boundary_width, default=0, metavar='D', help='also score contours: Boundary IoU (Cheng et al.) and trimap mIoU of the pixels within '
                   'D pixels (1..32, a Chebyshev band) of a class border, one kernel per batch (DESIGN.md section 12c); saved as bcounts_<seed>.npy and '
                   'band_cmatrix_<seed>.npy; 0 = off')
    p.add_argument('--allow-random-init', action='store_true', help='evaluate random weights when --restore-from does not exist')
    return p


def boundary_width(text):
    """--boundary-width: an integer in 0..32 (0 = off; sl_boundary_counts takes bands of 1..32 pixels)."""
    try:
        d = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--boundary-width %r is not an integer' % (text,))
    if not 0 <= d <= 32:
        raise argparse.ArgumentTypeError('--boundary-width %d is outside 0..32 pixels (0 = off; the band kernel holds widths up to 32)' % d)
    return d


def label_grid(label, ignore_label, pad_to_longside=False):
    """(label, size) the prediction is scored at: the label as it is, or (eval_ft.py:166-181) padded with ignore to a square of its long side."""
    h, w = label.shape[-2:]
    if not pad_to_longside:
        return label, (h, w)
    side = max(h, w)
    pad = torch.full((label.shape[0], side, side), ignore_label, dtype=label.dtype, device=label.device)
    pad[:, :h, :w] = label
    return pad, (side, side)


def confusion_of_batch(logits, label, num_classes, ignore_label, pad_to_longside=False):
    """eval_base.py:166-177 (eval_ft.py:166-181 with pad_to_longside): prediction at the label grid and its confusion counts."""
    label, size = label_grid(label, ignore_label, pad_to_longside)
    pred = ops.upsample_argmax(logits.float().contiguous(), size)
    return pred, ops.confusion_matrix(pred, label.contiguous(), num_classes, ignore_label)


def write_prediction_tiff(path, pred_hw, source_tif=None):
    """eval_base.py:180-188: the label map of one tile as a single-band uint8 TIFF with the class colormap.  With rasterio installed and the tile's source image at hand
    the file is the reference's GeoTIFF (the source's profile -- CRS, transform -- with driver GTiff, dtype uint8, count 1, nodata 0, + write_colormap); without rasterio
    (the build image) Pillow writes the same pixels and the same palette as a baseline palette TIFF, without georeferencing.  Returns 'rasterio' or 'PIL'."""
    from .fusemat import COLORMAP
    pred_hw = np.ascontiguousarray(pred_hw, dtype=np.uint8)
    try:
        import rasterio
    except ImportError:
        rasterio = None
    if rasterio is not None and source_tif is not None and osp.exists(source_tif):
        with rasterio.open(source_tif) as src:
            profile = src.profile.copy()
        profile.update(driver='GTiff', dtype='uint8', count=1, nodata=0)
        with rasterio.open(path, 'w', **profile) as f:
            f.write(pred_hw, 1)
            f.write_colormap(1, {i: tuple(int(v) for v in COLORMAP[i % len(COLORMAP)]) for i in range(256)})
        return 'rasterio'
    from PIL import Image
    img = Image.fromarray(pred_hw, 'P')
    img.putpalette(np.resize(COLORMAP, (256, 3)).astype(np.uint8).tobytes())
    img.save(path, format='TIFF')
    return 'PIL'


def dump_probabilities(logits, size, pred, ids, out_dir, data_dir=None):
    """eval_base.py:168,180-190: per tile `<id>.mat` = {'outputs': [1,K,H,W] logits upsampled with align_corners=True} (the input of fusemat.py), `<id>.tif` = the
    argmax as a colormapped single-band TIFF next to the .mat directory (write_prediction_tiff: the reference's GeoTIFF when rasterio and the source tile
    <data_dir>/image/<id>.tif exist), and `<id>.png`, the same as a palette image."""
    dump_maps(ops.upsample_logits(logits.float().contiguous(), tuple(size)), size, pred, ids, out_dir, data_dir)


def dump_maps(up, size, pred, ids, out_dir, data_dir=None):
    """The files of dump_probabilities from a ready [B,K,H,W] map: the upsampled logits, or the fused map of the test-time augmentation (cut to `size`)."""
    import scipy.io
    from .fusemat import COLORMAP
    os.makedirs(out_dir, exist_ok=True)
    up = up[:, :, :size[0], :size[1]].cpu().numpy()
    pred = pred.cpu().numpy()
    for b in range(up.shape[0]):
        name = str(ids[b].item() if hasattr(ids[b], 'item') else ids[b])
        scipy.io.savemat(osp.join(out_dir, name + '.mat'), {'outputs': up[b:b + 1]})
        try:
            os.makedirs(out_dir + '_tif', exist_ok=True)
            write_prediction_tiff(osp.join(out_dir + '_tif', name + '.tif'), pred[b][:size[0], :size[1]],
                                  osp.join(data_dir, 'image', name + '.tif') if data_dir else None)
        except ImportError:
            pass
        try:
            from PIL import Image
            img = Image.fromarray(pred[b][:size[0], :size[1]], 'P')
            img.putpalette(np.resize(COLORMAP, (256, 3)))
            os.makedirs(out_dir + '_png', exist_ok=True)           # next to, not inside, the .mat directory fusemat walks
            img.save(osp.join(out_dir + '_png', name + '.png'))
        except ImportError:
            pass


def miou_from_confusion(cm, n_base):
    """eval_base.py:193-199: per-class IoU = tp / (row + column - tp); base = classes 0..n_base, novel = the rest."""
    cm = np.asarray(cm, dtype=np.float64)
    pos, res, tp = cm.sum(1), cm.sum(0), np.diag(cm)
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = tp / (pos + res - tp)
    return iou, float(np.nanmean(iou[:n_base + 1])), float(np.nanmean(iou[n_base + 1:])) if len(iou) > n_base + 1 else float('nan'), float(np.nanmean(iou))


def boundary_iou_from_counts(counts, n_base):
    """Boundary IoU per class from the [3][K] counts of ops.boundary_counts: intersection / (ground-truth band + prediction band - intersection), NaN for a class with
    neither band; base / novel / total means over the class ranges of miou_from_confusion."""
    counts = np.asarray(counts, dtype=np.float64)
    inter, gt, pr = counts
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = inter / (gt + pr - inter)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                 # nanmean of an all-NaN range is NaN, which is the answer
        return iou, float(np.nanmean(iou[:n_base + 1])), float(np.nanmean(iou[n_base + 1:])) if len(iou) > n_base + 1 else float('nan'), float(np.nanmean(iou))


def predict_plain(model, image, size, map_size=None):
    """The single-view predictor (eval_base.py:166-168): the forward under no_grad, then upsampling + argmax to `size` in one kernel and, when a map is wanted, the logits
    upsampled to `map_size`.  -> (labels uint8 [B,H,W], float [B,K,map_size] or None)."""
    with torch.no_grad():
        logits = model(image).float().contiguous()
    return ops.upsample_argmax(logits, size), ops.upsample_logits(logits, tuple(map_size)) if map_size is not None else None


def select_predictor(args):
    """(predict, describe) for the parsed flags: plain, test-time augmentation or sliding windows; the latter two together are refused.  Every predict has the call shape of
    predict_plain; the fusing ones give their map on `size` itself and read `map_size` as 'a map is wanted'.  describe(image size, size) is the log line of the first
    batch, None for the plain predictor."""
    scales = tta.parse_scales(args.tta_scales)
    crop, stride = slide.driver_geometry(args.slide_crop, args.slide_stride)
    if slide.is_on(crop) and tta.is_on(scales, args.tta_flip):
        raise ValueError('--slide-crop together with --tta-scales / --tta-flip: windows of augmented views are not implemented; use one of the two')
    if slide.is_on(crop):
        def predict(model, image, size, map_size=None):
            if tuple(size) != tuple(image.shape[-2:]):
                raise ValueError('--slide-crop: the prediction is scored at %dx%d but the image is %dx%d; windows are cut from the image, so the two grids must be the same'
                                 % (tuple(size) + tuple(image.shape[-2:])))
            return slide.predict(model, image, crop, stride, mode=args.slide_mode, blend=args.slide_blend, want_map=map_size is not None, batch=args.slide_batch)
        def describe(hw, size):
            (ch, ys), (cw, xs) = slide.window_grid(hw[0], crop[0], stride[0]), slide.window_grid(hw[1], crop[1], stride[1])
            return 'sliding-window inference: %d windows per tile (%d x %d of %dx%d on %dx%d), crop %dx%d, stride %dx%d, blend %s, mode %s' % (
                len(ys) * len(xs), len(ys), len(xs), ch, cw, hw[0], hw[1], crop[0], crop[1], stride[0], stride[1], args.slide_blend, args.slide_mode)
        return predict, describe
    if tta.is_on(scales, args.tta_flip):
        def predict(model, image, size, map_size=None):
            return tta.predict(model, image, size, scales=scales, flip=args.tta_flip, mode=args.tta_mode, want_map=map_size is not None)
        def describe(hw, size):
            sizes = tta.view_sizes(hw[0], hw[1], scales)
            return 'test-time augmentation: %d views per tile (images %s%s), mode %s, fused at %dx%d' % (
                len(sizes) * (2 if args.tta_flip else 1), ', '.join('%dx%d' % s for s in sizes), '; each plain and mirrored' if args.tta_flip else '', args.tta_mode, size[0], size[1])
        return predict, describe
    return predict_plain, None


def main(argv=None, ft=False):
    parser = get_parser()
    with Engine(custom_parser=parser, argv=argv) as engine:
        args = engine.args
        logger = None
        if engine.is_main and args.save_path:
            os.makedirs(args.save_path, exist_ok=True)
            from datetime import datetime
            logger = my_utils.get_logger('', args.save_path, datetime.now().strftime('%Y_%m_%d_%H_%M_%S'))
        args.base_size = tuple(map(int, args.base_size.split(',')))
        predict, describe = select_predictor(args)
        ds = resolve(dataset_pkg, args.dataset)
        testset = ds.GFSSegVal(args.data_dir, args.val_list, args.fold, base_size=args.base_size, resize_label=False, use_novel=True, use_base=True)
        test_loader, test_sampler = engine.get_test_loader(testset)
        args.ignore_label = testset.ignore_label
        args.base_classes, args.novel_classes = len(testset.base_classes), len(testset.novel_classes)
        args.num_classes = testset.num_classes + 1                      # background counts as a class (eval_base.py:120)
        if engine.distributed:
            test_sampler.set_epoch(0)
        assert args.os in (8, 16, 32)
        model_cls = getattr(networks, args.model).GFSS_Model
        seg_model = model_cls(n_base=args.base_classes, backbone=args.backbone, dilated=(args.os != 32), os=args.os,
                              n_novel=args.novel_classes, is_ft=ft, compute_dtype=compute_dtype(args))
        model = engine.data_parallel(seg_model.to(engine.device))
        results = {}
        for seed in map(int, args.random_seed.split(',')):
            path = (args.restore_from[:-4] + '_%d.pth' % seed) if ft else args.restore_from       # eval_ft.py:154
            if checkpoint_or_none(path, args.allow_random_init):
                my_utils.load_model(model, path)
            model.eval()
            cm = torch.zeros((args.num_classes, args.num_classes), dtype=torch.int64, device=engine.device)
            bd = args.boundary_width                                    # 0 = off: no buffer, no launch, nothing saved or logged below
            bcounts = torch.zeros((3, args.num_classes), dtype=torch.int64, device=engine.device) if bd else None
            band_cm = torch.zeros_like(cm) if bd else None
            dump_dir = osp.join(args.save_path, 'prob_%d' % seed) if args.save_prob and args.save_path else None
            for batch in test_loader:
                # ready tensors (synthetic) or raw uint8 tiles + draws prepared on the GPU (oem / synthetic_raw: Engine installs raw_collate)
                image, label = batch_to_device(batch, testset, engine.device)
                # the tile's own size and the grid the prediction is scored at; unlabeled test tiles (eval_base.py:178-191): nothing to score, prediction and dump are the product
                tile = tuple((image if label is None else label).shape[-2:])
                label_p, size = (None, tile) if label is None else label_grid(label, args.ignore_label, pad_to_longside=ft)
                # The map is asked for at the tile's size.  predict_plain upsamples the logits to exactly that (the reference's .mat), although its labels are taken at `size`;
                # the fusing predictors give their map on `size` and dump_maps cuts it to the tile.  The two coincide unless eval_ft pads a non-square tile; each is kept as it is.
                pred, out_map = predict(model, image, size, tile if dump_dir else None)
                if describe is not None and engine.is_main:
                    (logger.info if logger else print)(describe(tuple(image.shape[-2:]), size))
                    describe = None
                if label is not None:
                    label_p = label_p.contiguous()
                    cm += ops.confusion_matrix(pred, label_p, args.num_classes, args.ignore_label)
                    if bd:
                        c, b = ops.boundary_counts(pred, label_p, args.num_classes, args.ignore_label, bd)
                        bcounts += c
                        band_cm += b
                if out_map is not None:
                    dump_maps(out_map, tile, pred, batch[2], dump_dir, data_dir=getattr(args, 'data_dir', None))
            if engine.distributed:
                cm = engine.all_reduce_tensor(cm, norm=False)
                if bd:
                    bcounts, band_cm = engine.all_reduce_tensor(bcounts, norm=False), engine.all_reduce_tensor(band_cm, norm=False)
            cmn = cm.cpu().numpy().astype(np.float64)
            iou, base_miou, novel_miou, total_miou = miou_from_confusion(cmn, args.base_classes)
            results[seed] = (base_miou, novel_miou, total_miou)
            if engine.is_main:
                if args.save_path:
                    np.save(osp.join(args.save_path, 'cmatrix_%d.npy' % seed), cmn)
                msg = ['>>>>>>> Current Seed %d: <<<<<<<' % seed, 'meanIoU---base: mIoU %.4f.' % base_miou,
                       'meanIoU---novel: mIoU %.4f.' % novel_miou, 'meanIoU---total: mIoU %.4f.' % total_miou]
                if bd:
                    bcn, bcmn = bcounts.cpu().numpy().astype(np.float64), band_cm.cpu().numpy().astype(np.float64)
                    if args.save_path:
                        np.save(osp.join(args.save_path, 'bcounts_%d.npy' % seed), bcn)
                        np.save(osp.join(args.save_path, 'band_cmatrix_%d.npy' % seed), bcmn)
                    for name, (_, b, n, t) in (('boundaryIoU', boundary_iou_from_counts(bcn, args.base_classes)), ('trimapIoU', miou_from_confusion(bcmn, args.base_classes))):
                        msg += ['%s(d=%d)---%s: mIoU %.4f.' % (name, bd, part, v) for part, v in (('base', b), ('novel', n), ('total', t))]
                for m in msg:
                    (logger.info if logger else print)(m)
        return results


if __name__ == '__main__':
    main()
