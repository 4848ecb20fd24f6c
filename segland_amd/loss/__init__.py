from .criterion import OrthLoss


def get_loss(args):
    """loss/__init__.py:3-8 of the reference: POP models train with OrthLoss.  args.class_weights (a sequence of floats, or the drivers' comma-separated string; empty:
    none) and args.label_smoothing are the weight / label_smoothing of the criterion's CrossEntropyLoss; args.dice_weight > 0 adds that multiple of the multiclass soft
    Dice loss (OrthLoss); args.ohem_thresh > 0 turns on online hard-pixel mining with that threshold and args.ohem_min_kept pixels kept at least (OrthLoss);
    args.focal_gamma >= 1 makes the cross-entropy a focal loss with that exponent (0: off; OrthLoss); args.lovasz_weight > 0 adds that multiple of the Lovasz-softmax
    loss (OrthLoss).  A namespace without them gets the reference's plain loss."""
    if 'pop' in args.model:
        weights = getattr(args, 'class_weights', None)
        if isinstance(weights, str):
            from ..drivers import class_weights
            weights = class_weights(weights)
        weights = None if weights is None or len(weights) == 0 else weights
        return OrthLoss(ignore_index=args.ignore_label, weight=weights, label_smoothing=getattr(args, 'label_smoothing', 0.0),
                        dice_weight=getattr(args, 'dice_weight', 0.0), ohem_thresh=getattr(args, 'ohem_thresh', None) or None,
                        ohem_min_kept=getattr(args, 'ohem_min_kept', 100000), focal_gamma=getattr(args, 'focal_gamma', 0.0),
                        lovasz_weight=getattr(args, 'lovasz_weight', 0.0))
    raise RuntimeError('segland_amd implements the POP path only (model %r): CELoss models are out of scope' % (args.model,))
