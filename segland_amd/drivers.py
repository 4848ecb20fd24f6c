"""Shared pieces of the two training entry points (train_base.py / ft_pop.py of the reference): the command-line
surface, LR schedule, validation loop and checkpoint writer.  The flag names, defaults and meanings are the reference's
(train_base.py:47-111, ft_pop.py:47-115) so scripts/*.sh work with only the module path edited."""
import argparse
import os

import numpy as np
import torch

from .utils import pyt_utils as my_utils


def str2bool(v):
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


def class_weights(v):
    """'' -> () (no weights); '1,0.5,2' -> (1.0, 0.5, 2.0).  One finite, non-negative value per logit channel (the count is checked against the model's channels
    by OrthLoss, which knows them)."""
    if isinstance(v, (tuple, list)):
        return tuple(float(x) for x in v)
    if not v.strip():
        return ()
    try:
        w = tuple(float(x) for x in v.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('comma-separated floats expected, one per logit channel (got %r)' % (v,))
    if not all(np.isfinite(x) and x >= 0.0 for x in w):
        raise argparse.ArgumentTypeError('class weights must be finite and non-negative (got %r)' % (v,))
    return w


def label_smoothing(v):
    try:
        eps = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError('float expected (got %r)' % (v,))
    if not 0.0 <= eps <= 1.0:
        raise argparse.ArgumentTypeError('label smoothing must lie in [0, 1] (got %r)' % (v,))
    return eps


def dice_weight(v):
    try:
        lam = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError('float expected (got %r)' % (v,))
    if not (np.isfinite(lam) and lam >= 0.0):
        raise argparse.ArgumentTypeError('the Dice weight must be finite and >= 0 (got %r)' % (v,))
    return lam


def ohem_thresh(v):
    try:
        th = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError('float expected (got %r)' % (v,))
    if not 0.0 <= th <= 1.0:
        raise argparse.ArgumentTypeError('the hard-pixel mining threshold must lie in (0, 1], or be 0 for off (got %r)' % (v,))
    return th


def ohem_min_kept(v):
    try:
        n = int(v)
    except ValueError:
        raise argparse.ArgumentTypeError('integer expected (got %r)' % (v,))
    if n < 1:
        raise argparse.ArgumentTypeError('the number of pixels hard-pixel mining keeps at least must be >= 1 (got %r)' % (v,))
    return n


def focal_gamma(v):
    try:
        gamma = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError('float expected (got %r)' % (v,))
    if gamma != 0.0 and not (np.isfinite(gamma) and gamma >= 1.0):
        raise argparse.ArgumentTypeError('the focal exponent must be finite and >= 1, or 0 for off (got %r)' % (v,))
    return gamma


def lovasz_weight(v):
    try:
        lam = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError('float expected (got %r)' % (v,))
    if not (np.isfinite(lam) and lam >= 0.0):
        raise argparse.ArgumentTypeError('the Lovasz weight must be finite and >= 0 (got %r)' % (v,))
    return lam


def aug_scale(v):
    """--aug-scale: '' -> () (off); 'LO,HI' -> (lo, hi) with 0 < LO <= HI <= 4: the range the random rescale before the crop is drawn from."""
    if isinstance(v, (tuple, list)):
        return tuple(float(x) for x in v)
    if not v.strip():
        return ()
    try:
        r = tuple(float(x) for x in v.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('two comma-separated floats LO,HI expected (got %r)' % (v,))
    if len(r) != 2 or not (0.0 < r[0] <= r[1] <= 4.0):
        raise argparse.ArgumentTypeError('the rescale range LO,HI must satisfy 0 < LO <= HI <= 4 (got %r)' % (v,))
    return r


def aug_jitter(v):
    """--aug-jitter: '' -> () (off); 'B,C,S' -> the brightness, contrast and saturation amplitudes, each in [0, 1)."""
    if isinstance(v, (tuple, list)):
        return tuple(float(x) for x in v)
    if not v.strip():
        return ()
    try:
        a = tuple(float(x) for x in v.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('three comma-separated floats B,C,S expected (got %r)' % (v,))
    if len(a) != 3 or not all(0.0 <= x < 1.0 for x in a):
        raise argparse.ArgumentTypeError('the jitter amplitudes B,C,S (brightness, contrast, saturation) must each lie in [0, 1) (got %r)' % (v,))
    return a


def aug_rotate(v):
    """--aug-rotate: '' -> () (off); 'LO,HI[,P]' -> (lo, hi, p): the range in degrees the rotation about the crop centre is drawn from, -180 <= LO <= HI <= 180, applied with
    probability P in (0, 1] (default 0.5, as the reference's random_rotate)."""
    if isinstance(v, (tuple, list)):
        return tuple(float(x) for x in v)
    if not v.strip():
        return ()
    try:
        r = tuple(float(x) for x in v.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('comma-separated floats LO,HI[,P] expected (got %r)' % (v,))
    if len(r) == 2:
        r += (0.5,)
    if len(r) != 3 or not (-180.0 <= r[0] <= r[1] <= 180.0) or not (0.0 < r[2] <= 1.0):
        raise argparse.ArgumentTypeError('the rotation range LO,HI[,P] must satisfy -180 <= LO <= HI <= 180 and 0 < P <= 1 (got %r)' % (v,))
    return r


def aug_blur(v):
    """--aug-blur: '' -> () (off); 'K[,P]' -> (K, p): the odd size 3, 5, 7, 9 or 11 of the Gaussian blur, applied with probability P in (0, 1] (default 0.5, as the
    reference's random_gaussian)."""
    if isinstance(v, (tuple, list)):
        return tuple(int(x) if i == 0 else float(x) for i, x in enumerate(v))
    if not v.strip():
        return ()
    try:
        a = tuple(float(x) for x in v.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('an odd size and an optional probability K[,P] expected (got %r)' % (v,))
    if len(a) == 1:
        a += (0.5,)
    if len(a) != 2 or a[0] not in (3.0, 5.0, 7.0, 9.0, 11.0) or not (0.0 < a[1] <= 1.0):
        raise argparse.ArgumentTypeError('the blur K[,P] needs an odd K in 3..11 and 0 < P <= 1 (got %r)' % (v,))
    return (int(a[0]), a[1])


def _augment_flags(args):
    return (('--aug-scale', 'scale', aug_scale(getattr(args, 'aug_scale', ()) or ())), ('--aug-jitter', 'jitter', aug_jitter(getattr(args, 'aug_jitter', ()) or ())),
            ('--aug-rotate', 'rotate', aug_rotate(getattr(args, 'aug_rotate', ()) or ())), ('--aug-blur', 'blur', aug_blur(getattr(args, 'aug_blur', ()) or ())))


def augment_option(args, reader, dataset):
    """The `augment=` keyword of a training reader from --aug-scale / --aug-jitter / --aug-rotate / --aug-blur: {} when all are off (the reader is called as it always was), else
    {'augment': {'scale': ..., 'jitter': ...}}, with the keys 'rotate' / 'blur' only when their flag is on.  A reader that does not hand raw tiles to the GPU preparation kernel
    cannot take the option: a ValueError names it and the flags."""
    flags = _augment_flags(args)
    if not any(on for _, _, on in flags):
        return {}
    if not getattr(reader, 'accepts_augment', False):
        raise ValueError("dataset '%s' cannot take %s: its training reader does not emit raw tiles for the GPU preparation kernel (csrc/augment.hip); "
                         'use oem, synthetic_tiff or synthetic_raw' % (dataset, ' / '.join(f for f, _, on in flags if on)))
    return {'augment': {key: on or None for _, key, on in flags if on or key in ('scale', 'jitter')}}


def log_augment_options(args):
    """One line at start, only when one of the four augmentation flags is on; it names the ones that are."""
    scale, jitter, rotate, blur = (on for _, _, on in _augment_flags(args))
    parts = ((' random rescale %g..%g before the crop' % scale if scale else ''), (' colour jitter: brightness %g, contrast %g, saturation %g' % jitter if jitter else ''),
             (' rotation by %g..%g degrees about the crop centre (probability %g)' % rotate if rotate else ''), (' %dx%d Gaussian blur (probability %g)' % (blur[0], blur[0], blur[1]) if blur else ''))
    if any(parts):
        import logging
        logging.getLogger('Segmentation').info('tile augmentation in the preparation kernel:' + ','.join(p for p in parts if p))


def ema_decay(v):
    """--ema-decay: 0 (off) or a decay in (0, 1); anything else -- NaN included -- is a ValueError that holds the value.  Not an argparse `type`: argparse would turn
    the error into its own exit message."""
    d = float(v)
    if d != 0.0 and not 0.0 < d < 1.0:
        raise ValueError('--ema-decay must be 0 (off) or lie strictly between 0 and 1 (got %r)' % (v,))
    return d


def make_ema(args, model, optimizer, log=False):
    """The weight average of a run (segland_amd/ema.py) attached to its optimizer, or None when --ema-decay is 0.  `model`: the wrapped model, on its device and in the
    mode it trains in (the tracked set is fixed here).  The update rides on the step of a segland_amd.optim optimizer; torch's optimizers have no such hook."""
    d = ema_decay(getattr(args, 'ema_decay', 0.0))
    if d == 0.0:
        return None
    if not hasattr(optimizer, 'attach_ema'):
        raise ValueError('--ema-decay %g: the weight average is updated by a kernel behind the step of segland_amd.optim.AdamW / SGD (the GPU path); %s.%s has no '
                         'such hook (no GPU?)' % (d, type(optimizer).__module__, type(optimizer).__name__))
    from .ema import ModelEma
    ema = ModelEma(model, d, warmup=getattr(args, 'ema_warmup', True))
    optimizer.attach_ema(ema)
    if log:
        import logging
        logging.getLogger('Segmentation').info('weight EMA: decay %g%s, %d tensors (%d values) averaged after every step; validation, best and *_ema checkpoints use the average',
                                               d, ' with warm-up min(decay, (1 + t) / (10 + t))' if ema.warmup else '', len(ema.names),
                                               sum(s.numel() for s in ema.shadows.values()))
    return ema


def averaged(ema):
    """Context of a validation: the averaged weights stand in the model (ModelEma.applied), or nothing changes without an EMA."""
    import contextlib
    return ema.applied() if ema is not None else contextlib.nullcontext()


def save_ema_checkpoint(ema, path):
    """The averaged weights in the format of save_checkpoint (eval_base / eval_ft load the file unchanged)."""
    torch.save(ema.model_state_dict(), path, _use_new_zipfile_serialization=False)


def log_loss_options(args):
    """One line at start: the controls of the segmentation criterion (loss.get_loss reads the same fields); the Dice weight, the focal exponent, the Lovasz weight and the mining controls only where they are on."""
    import logging
    w = class_weights(getattr(args, 'class_weights', ()) or ())
    lam = float(getattr(args, 'dice_weight', 0.0))
    th = float(getattr(args, 'ohem_thresh', 0.0) or 0.0)
    gamma = float(getattr(args, 'focal_gamma', 0.0))
    lov = float(getattr(args, 'lovasz_weight', 0.0))
    logging.getLogger('Segmentation').info('segmentation loss: class weights %s, label smoothing %g' + (', dice weight %g' if lam > 0.0 else '')
                                           + (', focal gamma %g' if gamma > 0.0 else '')
                                           + (', lovasz weight %g' if lov > 0.0 else '')
                                           + (', hard-pixel mining: threshold %g, at least %d pixels per batch' if th > 0.0 else ''),
                                           ','.join('%g' % x for x in w) if w else 'none', float(getattr(args, 'label_smoothing', 0.0)), *((lam,) if lam > 0.0 else ()),
                                           *((gamma,) if gamma > 0.0 else ()), *((lov,) if lov > 0.0 else ()),
                                           *((th, int(getattr(args, 'ohem_min_kept', 100000))) if th > 0.0 else ()))


# (flag, kwargs) -- common to both drivers
_COMMON = [
    ('--dataset', dict(type=str, default='cityscapes', help='Dataset for training')),
    ('--batch-size', dict(type=int, default=8, help='Number of images sent to the network in one step.')),
    ('--data-dir', dict(type=str, default='/data/pascal-context', help='Path to the dataset directory.')),
    ('--train-list', dict(type=str, default='./dataset/list/context/train.txt', help='File listing the training images.')),
    ('--base-size', dict(type=str, default='1024,1024', help='Base size of images for resize.')),
    ('--input-size', dict(type=str, default='512,512', help='Comma-separated height,width of the training crops.')),
    ('--learning-rate', dict(type=float, default=1e-2, help='Base learning rate (polynomial decay).')),
    ('--momentum', dict(type=float, default=0.9, help='Momentum component of the optimiser.')),
    ('--power', dict(type=float, default=0.9, help='Decay parameter of the learning rate.')),
    ('--weight-decay', dict(type=float, default=0.0005, help='Regularisation parameter for L2-loss.')),
    ('--start-epoch', dict(type=int, default=0, help='Which epoch to start.')),
    ('--num-epoch', dict(type=int, default=100, help='Number of training epochs.')),
    ('--restore-from', dict(type=str, default='/home/model/resnet_backbone/resnet101-imagenet.pth', help='Where to restore model parameters from.')),
    ('--snapshot-dir', dict(type=str, default='/home/output', help='Where to save snapshots of the model.')),
    ('--model', dict(type=str, default='None', help='choose model.')),
    ('--num-workers', dict(type=int, default=4, help='choose the number of workers.')),
    ('--backbone', dict(type=str, default='resnet50', help='backbone model: resnet101, resnet50 (default)')),
    ('--os', dict(type=int, default=8, help='output stride')),
    ('--print-frequency', dict(type=int, default=100, help='Number of training steps between log lines.')),
    ('--save-pred-every', dict(type=int, default=5, help='Save summaries and checkpoint every often.')),
    ('--shot', dict(type=int, default=1, help='number of support pairs')),
    ('--val-list', dict(type=str, default='./dataset/list/context/val.txt', help='File listing the validation images.')),
    ('--test-batch-size', dict(type=int, default=1, help='Number of images sent to the network in one validation step.')),
    ('--filter-novel', dict(action='store_true', default=False, help='filter images containing novel classes during training.')),
    ('--freeze-backbone', dict(action='store_true', default=False, help='freeze the backbone during training.')),
    ('--no-step-graph', dict(action='store_true', default=False, help='issue every kernel of the training step from Python instead of replaying '
                                 'the step as one captured HIP graph (segland_amd/graph_step.py; single-GPU AdamW runs only).')),
    ('--allow-random-init', dict(action='store_true', default=False, help='continue with random weights when --restore-from does not exist '
                                                                           '(the reference fails in torch.load; so does this build without the flag).')),
    ('--class-weights', dict(type=class_weights, default='', help='comma-separated class weights of the segmentation cross-entropy, one per logit channel '
                                                                  '(1 + base classes; 1 + base + novel classes when fine-tuning); default: none.')),
    ('--label-smoothing', dict(type=label_smoothing, default=0.0, help='label smoothing of the segmentation cross-entropy, in [0, 1]; default 0.')),
    ('--dice-weight', dict(type=dice_weight, default=0.0, help='weight of the multiclass soft Dice term added to the segmentation cross-entropy (main and auxiliary '
                                                               'head; class weights scale its per-class terms, ignored pixels are left out); default 0: cross-entropy only.')),
    ('--focal-gamma', dict(type=focal_gamma, default=0.0, help='focal loss: every pixel\'s segmentation cross-entropy is scaled by (1 - p_t)^gamma, p_t the probability of its '
                                                               'label (main and auxiliary head; class weights are the focal alpha; with --dice-weight the Dice term is left '
                                                               'as it is); finite and >= 1; default 0: off.')),
    ('--lovasz-weight', dict(type=lovasz_weight, default=0.0, help='weight of the Lovasz-softmax term (the convex surrogate of the Jaccard index, over the classes present '
                                                                   'in the batch; binned, no sort) added to the segmentation loss of the main and the auxiliary head; '
                                                                   'class weights do not enter it; finite and >= 0; default 0: off.')),
    ('--ohem-thresh', dict(type=ohem_thresh, default=0.0, help='online hard-pixel mining (bootstrapped cross-entropy): only pixels whose probability of the true class '
                                                               'is at most this threshold, in (0, 1], enter the segmentation loss of a head, but never fewer than '
                                                               '--ohem-min-kept of them; default 0: off.')),
    ('--ohem-min-kept', dict(type=ohem_min_kept, default=100000, help='pixels per GPU batch that hard-pixel mining keeps at least (the hardest ones); default 100000.')),
    ('--aug-scale', dict(type=aug_scale, default='', help='LO,HI: every training tile is rescaled (bilinear; labels nearest) by a random factor from this range before the crop '
                                                          'is taken, inside the tile preparation kernel; 0 < LO <= HI <= 4 (PSPNet: 0.5,2.0); raw-tile datasets only; default: off.')),
    ('--aug-jitter', dict(type=aug_jitter, default='', help='B,C,S: random brightness, contrast and saturation of every training crop, inside the tile preparation kernel; '
                                                            'the amplitudes, each in [0, 1) (0.2,0.2,0.2 is common); raw-tile datasets only; default: off.')),
    ('--aug-rotate', dict(type=aug_rotate, default='', help='LO,HI[,P]: with probability P (default 0.5) every training crop is rotated about its centre by an angle in degrees '
                                                            'from this range (image bilinear, labels nearest, border 0 / ignore), inside the tile preparation kernel; '
                                                            '-180 <= LO <= HI <= 180 (the reference: -10,10); raw-tile datasets only; default: off.')),
    ('--aug-blur', dict(type=aug_blur, default='', help='K[,P]: with probability P (default 0.5) every training crop gets a K x K Gaussian blur (sigma from K by the rule of '
                                                        'OpenCV, reflect-101 border), inside the tile preparation kernel; K in 3, 5, 7, 9, 11 (the reference: 5); raw-tile '
                                                        'datasets only; default: off.')),
    ('--ema-decay', dict(type=float, default=0.0, help='exponential moving average of the trainable weights and the training BatchNorm statistics, updated after every '
                                                       'optimizer step; validation and best.pth use the average, epoch_N_ema.pth holds it next to the raw epoch_N.pth; '
                                                       'strictly between 0 and 1 (0.999 is common); default 0: off.')),
    ('--ema-warmup', dict(type=str2bool, default=True, help='the decay of step t is min(--ema-decay, (1 + t) / (10 + t)); default True.')),
    ('--fp16', dict(action='store_true', default=False, help='mixed precision: bf16 MFMA with fp32 accumulate on MI355X '
                                                                '(the reference uses fp16 autocast + GradScaler); default is exact-fp32 MFMA.')),
]
_BASE_ONLY = [
    ('--random-seed', dict(type=int, default=321, help='Random seed to have reproducible results.')),
    ('--fold', dict(type=int, default=0, choices=[-1, 0, 1, 2, 3], help='validation fold')),
    ('--fix-bn', dict(action='store_true', default=False, help='whether to fix batchnorm during training.')),
    ('--finetune', dict(action='store_true', default=False, help='whether to finetune the decoder.')),
    ('--single-step', dict(action='store_true', default=False, help='ONE AdamW step per iteration; default mirrors the reference, '
                                                                      'whose scaler.step + optimizer.step is two (train_base.py:262-264).')),
]
_FT_ONLY = [
    ('--random-seed', dict(type=str, default='123,234', help='Comma-separated seeds; one fine-tune run per seed.')),
    ('--fold', dict(type=int, default=0, choices=[0, 1, 2, 3], help='validation fold')),
    ('--fix-bn', dict(action='store_true', default=True, help='whether to fix batchnorm during training.')),
    ('--update-base', dict(action='store_true', default=False, help='whether to update base class with novel class.')),
    ('--update-epoch', dict(type=int, default=1, help='epoch interval for base-list update / validation.')),
    ('--fix-lr', dict(action='store_true', default=False, help='whether to fix learning rate during training.')),
]


def build_parser(ft=False):
    p = argparse.ArgumentParser(description='Few-shot Segmentation Framework (MI355X build)')
    for flag, kw in _COMMON + (_FT_ONLY if ft else _BASE_ONLY):
        p.add_argument(flag, **kw)
    return p


def lr_poly(base_lr, it, max_iter, power):
    return base_lr * ((1 - float(it) / max_iter) ** power)


def adjust_learning_rate_poly(optimizer, learning_rate, i_iter, max_iter, power, split=0, scale_lr=10.0):
    """Groups with index <= split get lr, the others lr*scale (train_base.py:116-128, ft_pop.py:119-131)."""
    lr = lr_poly(learning_rate, i_iter, max_iter, power)
    for index, group in enumerate(optimizer.param_groups):
        group['lr'] = lr if index <= split else lr * scale_lr
    return lr


def compute_dtype(args):
    return torch.bfloat16 if args.fp16 else torch.float32


_AUGMENTERS = None


def _augmenters_of(dataset):
    global _AUGMENTERS
    if _AUGMENTERS is None:
        import weakref
        _AUGMENTERS = weakref.WeakKeyDictionary()
    d = _AUGMENTERS.get(dataset)
    if d is None:
        d = _AUGMENTERS[dataset] = {}
    return d


def batch_to_device(batch, dataset, device):
    """(img, mask) on the device from a loader batch: ready tensors (synthetic), or raw uint8 tiles + the reference's random draws that the GPU
    crops / pads / flips / rotates / normalises / re-indexes in one launch (dataset/augment.py).  The augmenters (device-side lookup
    tables, ctypes staging) are cached per LIVE dataset object (_AUGMENTERS, weak keys): a cache keyed by id(dataset) would hand a later dataset that happens
    to get the same id the augmenter of a dead one (other crop size, statistics, label map); stored on the dataset itself they would be pickled into every
    DataLoader worker (the loaders are re-created every epoch; ctypes arrays do not pickle)."""
    if not getattr(dataset, 'raw_tiles', False):
        return batch[0].to(device, non_blocking=True), batch[1].to(device, non_blocking=True)
    tiles, params, _ = batch
    cache = _augmenters_of(dataset)
    if hasattr(dataset, 'crop_size'):
        key, make = ('train', str(device)), lambda: dataset.augmenter(device)
    else:                                  # validation: whole tiles, one augmenter per tile size
        size = tuple(tiles[0][0].shape[:2])
        key, make = (size, str(device)), lambda: dataset.augmenter(device, size)
    aug = cache.get(key)
    if aug is None:
        aug = cache[key] = make()
    return aug.prepare(tiles, params)


def ft_batch_to_device(batch, dataset, device):
    """(img, mask, img_b, mask_b) on the device from a fine-tune loader batch: ready tensors (synthetic_ft), or raw (novel, base) tile pairs +
    their draws (dataset/oem_ft.py, synthetic_raw_ft.py), whose 2B tiles are prepared by ONE GPU launch."""
    if not getattr(dataset, 'pair_tiles', False):
        return tuple(t.to(device, non_blocking=True) for t in batch[:4])
    cache = _augmenters_of(dataset)
    aug = cache.get(('pairs', str(device)))
    if aug is None:
        aug = cache[('pairs', str(device))] = dataset.augmenter(device)
    return aug.prepare(batch[0], batch[1])


def validate(model, dataloader, num_classes, ignore_label, device):
    """train_base.py:316-340 / ft_pop.py:312-336: logits -> upsample(align_corners=True) -> argmax -> IoU histogram,
    with the upsample+argmax fused in one HIP kernel (no H x W logits) and the histogram in another."""
    from . import ops
    model.eval()
    inter = torch.zeros(num_classes, device=device)
    union = torch.zeros(num_classes, device=device)
    for batch in dataloader:
        img, mask = batch_to_device(batch, dataloader.dataset, device)
        if mask is None:
            raise RuntimeError('validate(): the loader delivers unlabeled tiles; scoring needs labels (eval_base --save-prob dumps predictions for unlabeled tiles)')
        with torch.no_grad():
            logits = model(img)
            pred = ops.upsample_argmax(logits.float().contiguous(), mask.shape[1:])
        i, u, _ = my_utils.intersectionAndUnionGPU(pred, mask, num_classes, ignore_label)
        inter += i
        union += u
    return inter, union


def save_checkpoint(model, path):
    """Legacy (non-zipfile) serialisation and `module.`-prefixed keys, exactly the reference's on-disk format."""
    torch.save(model.state_dict(), path, _use_new_zipfile_serialization=False)


def save_training_state(model, optimizer, path, epoch, best=0.0, best_epoch=0, ema=None):
    """Everything a true resume needs (the reference saves the bare model state_dict only, train_base.py:286-292, and parses
    `-c/--continue` without using it, engine.py:62-65): model weights in the reference's `module.`-prefixed format under 'state_dict' (so
    utils.pyt_utils.load_model reads this file too), the optimizer state (torch.optim layout), the finished epoch and the best validation score;
    with a weight average (ema: segland_amd.ema.ModelEma) its state under 'ema'.  The weights under 'state_dict' are always the raw ones."""
    state = {'state_dict': model.state_dict(), 'optimizer': optimizer.state_dict(), 'epoch': int(epoch), 'best': float(best), 'best_epoch': int(best_epoch)}
    if ema is not None:
        state['ema'] = ema.state_dict()
    torch.save(state, path, _use_new_zipfile_serialization=False)


def load_training_state(model, optimizer, path, ema=None):
    """-> (epoch to continue with, best, best_epoch).  `model` is the wrapped model (its keys carry `module.`).  ema: restored from the file's 'ema'; a file written
    without one starts the average from the loaded weights."""
    ckpt = torch.load(path, map_location='cpu')
    if 'optimizer' not in ckpt or 'state_dict' not in ckpt:
        raise RuntimeError('%s is not a training state written by save_training_state (a bare state_dict restores weights only: use --restore-from)' % path)
    model.load_state_dict(ckpt['state_dict'], strict=True)
    optimizer.load_state_dict(ckpt['optimizer'])
    if ema is not None:
        if 'ema' in ckpt:
            ema.load_state_dict(ckpt['ema'])
        else:
            import logging
            logging.getLogger('Segmentation').warning('%s holds no weight average (written without --ema-decay): the average starts from the loaded weights', path)
            ema.reset_to_model()
    from .functional import weights_changed
    weights_changed()                      # the derived GEMM-layout weight copies follow the loaded parameters
    return int(ckpt['epoch']), float(ckpt.get('best', 0.0)), int(ckpt.get('best_epoch', 0))


def miou(inter, union):
    return np.nanmean((inter / union).cpu().numpy())


def checkpoint_or_none(path, allow_random_init, what='--restore-from'):
    """The path if it exists; None (random initialisation) only when explicitly allowed.  The reference raises inside torch.load for a
    missing file (utils/pyt_utils.py:91); silently training / evaluating a random model is never what the caller meant."""
    import os.path as osp
    if path and osp.exists(str(path)):
        return path
    if allow_random_init:
        import logging
        logging.getLogger('Segmentation').error('%s=%r does not exist: continuing with RANDOM weights (--allow-random-init)', what, path)
        return None
    raise FileNotFoundError('%s=%r does not exist (pass --allow-random-init to run with random weights)' % (what, path))


def resolve(dataset_pkg, name):
    mod = getattr(dataset_pkg, name, None)
    if mod is None:
        have = sorted(k for k, v in vars(dataset_pkg).items() if hasattr(v, 'GFSSegTrain'))
        raise RuntimeError("unknown dataset '%s' (available: %s; 'oem' / 'oem_ft' decode GeoTIFF tiles with rasterio or Pillow)" % (name, ', '.join(have)))
    return mod
