"""OrthLoss (loss/criterion.py:29-65 of the reference) with the bilinear upsample + cross-entropy fused in one HIP
kernel pair (the H x W logits are never materialised).  Returns the same dict of scalar tensors."""
import torch
import torch.nn as nn

from .. import ops
from ..functional import UpsampleCEDiceFn, UpsampleCEFn, UpsampleFocalDiceFn, UpsampleFocalFn, UpsampleLovaszFn


class OrthTerm:
    """The orthogonality term already evaluated by the model's fused prototype kernel (functional.ProtoFn), handed to OrthLoss in the place of
    the similarity matrix it would be computed from.  A plain tensor `proto_sim` still works (the reference's call)."""

    def __init__(self, value):
        self.value = value


class OrthLoss(nn.Module):
    """`weight` and `label_smoothing` are those of the nn.CrossEntropyLoss the reference builds its segmentation criterion from (loss/criterion.py:33), with torch's
    semantics; the main and the auxiliary loss both use them.  `weight` (one value per logit channel; 1 + n_base + n_novel of them in fine-tune mode) is kept as a float32
    NON-persistent buffer: it follows .to() / .cuda() and adds no key to a state_dict.  The kernels read the buffer itself, so an in-place update
    (criterion.weight.copy_(...)) reaches a captured training step without a new capture.

    `dice_weight` > 0 makes the segmentation criterion the hybrid one the reference keeps commented out beside its CrossEntropyLoss (loss/criterion.py:34,
    MulticlassHybridLoss): seg_loss = cross-entropy + dice_weight * Dice, with multiclass soft Dice on the softmax of the upsampled logits (sum over classes, each
    scaled by `weight` where given; mean over samples; `dice_smooth` in numerator and denominator; pixels with the ignore label enter neither term), for the main and
    the auxiliary head alike; the dict gains 'dice_loss', the main head's unscaled Dice term.  Both are plain floats: no buffer, no state_dict key.  dice_weight == 0
    is the code path without it.

    `ohem_thresh` (None or 0: off) turns on online hard-pixel mining (bootstrapped cross-entropy): per call and per head, only the valid pixels whose softmax probability
    of the true class is at most max(ohem_thresh, the ohem_min_kept-th smallest such probability) count -- every pixel at or below the threshold, and at least
    ohem_min_kept pixels (all of them when fewer are valid).  The head's criterion, cross-entropy and Dice term alike, is evaluated on the mined label map (the target
    with the dropped pixels set to ignore_index, in a new buffer: `target` is never written) by the same kernels; the kept set is a constant for the gradient.  Each
    head mines by its own probabilities; `weight` and `label_smoothing` do not enter them.  ohem_min_kept counts pixels per call (per GPU batch).  The dict gains
    'ohem_frac', the kept fraction of the main head's valid pixels (a device scalar; no read-back, so the step stays capturable).  Both are plain Python values: no
    buffer, no state_dict key.  Off is the code path without it.

    `focal_gamma` (0: off, else a finite value >= 1) makes the cross-entropy a focal loss (Lin et al.), the smooth counterpart of the mining's hard cut: every valid
    pixel's cross-entropy numerator is scaled by (1 - p_t)^focal_gamma, p_t the softmax probability of its label, computed as the sum of the other classes'
    exponentials over the sum of all (no cancellation near p_t = 1; exactly 0 once the other classes underflow), inside the same fused kernels, gradient included.
    The mean still divides by the cross-entropy's own denominator (the number, or with `weight` the weight sum, of the valid pixels), so `weight` acts as the focal
    alpha; label smoothing is modulated as a whole (the factor multiplies the smoothed numerator).  Values below 1 are refused: the gradient carries
    (1 - p_t)^(focal_gamma - 1), unbounded there.  With dice_weight > 0 only the cross-entropy part is modulated, the Dice term is unchanged; with mining on, the
    pixels are mined by the unmodulated probabilities first and the focal criterion runs on the mined label map; the auxiliary head uses the same criterion.  The dict
    gains no key: 'seg_loss' is the focal loss.  A plain float: no buffer, no state_dict key -- and, unlike the `weight` buffer, a kernel ARGUMENT: a captured
    training step bakes the value in, so changing focal_gamma needs a new capture.  focal_gamma == 0 is the code path without it.

    `lovasz_weight` > 0 (a finite value >= 0) adds that multiple of the Lovasz-softmax loss (Berman et al.), the convex surrogate of the Jaccard index the runs are
    scored by: seg_loss = cross-entropy [+ dice_weight * Dice] + lovasz_weight * Lovasz, for the main and the auxiliary head alike; the dict gains 'lovasz_loss', the
    main head's unscaled term.  Per call and per head (under DDP per rank), over the valid pixels of the whole batch: for every class PRESENT in the labels, the Lovasz
    extension of its Jaccard loss at the errors |[t == c] - p_c| of the softmax of the upsampled logits, mean over the present classes.  The kernels do not sort: the
    errors are quantised to 1024 bins (include/segland_hip.h), which moves the loss by at most 1 / 2048 from the sorted one, and the gradient is the bin-averaged
    subgradient.  No class weights on this term (`weight` does not enter it) and no per-image variant.  The cross-entropy (weighted, smoothed, focal) and the Dice term
    are those of the criterion without it, bit for bit; the backward is one launch for all terms.  With mining on, the term runs on the head's mined label map, like
    Dice.  A plain float: no buffer, no state_dict key.  lovasz_weight == 0 is the code path without it."""

    def __init__(self, ignore_index=255, reduction='mean', weight=None, label_smoothing=0.0, dice_weight=0.0, dice_smooth=1.0, ohem_thresh=None, ohem_min_kept=100000,
                 focal_gamma=0.0, lovasz_weight=0.0):
        super().__init__()
        if reduction != 'mean':
            raise ValueError('segland_amd OrthLoss implements reduction="mean" (what the reference uses)')
        label_smoothing = float(label_smoothing)
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError('OrthLoss: label_smoothing %r outside [0, 1]' % (label_smoothing,))
        dice_weight, dice_smooth = float(dice_weight), float(dice_smooth)
        if not 0.0 <= dice_weight < float('inf'):
            raise ValueError('OrthLoss: dice_weight %r is not a finite value >= 0' % (dice_weight,))
        if not 0.0 < dice_smooth < float('inf'):
            raise ValueError('OrthLoss: dice_smooth %r is not a finite value > 0' % (dice_smooth,))
        if ohem_thresh is not None:
            ohem_thresh = float(ohem_thresh)
            if ohem_thresh == 0.0:
                ohem_thresh = None
            elif not 0.0 < ohem_thresh <= 1.0:
                raise ValueError('OrthLoss: ohem_thresh %r outside (0, 1] (None or 0: off)' % (ohem_thresh,))
        if isinstance(ohem_min_kept, bool) or int(ohem_min_kept) != ohem_min_kept or int(ohem_min_kept) < 1:
            raise ValueError('OrthLoss: ohem_min_kept %r is not an integer >= 1' % (ohem_min_kept,))
        focal_gamma = float(focal_gamma)
        if focal_gamma != 0.0 and not 1.0 <= focal_gamma < float('inf'):
            raise ValueError('OrthLoss: focal_gamma %r is neither 0 (off) nor a finite value >= 1' % (focal_gamma,))
        lovasz_weight = float(lovasz_weight)
        if not 0.0 <= lovasz_weight < float('inf'):
            raise ValueError('OrthLoss: lovasz_weight %r is not a finite value >= 0' % (lovasz_weight,))
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).detach().clone().contiguous()
            if weight.dim() != 1 or weight.numel() == 0:
                raise ValueError('OrthLoss: weight must be a non-empty vector, one value per logit channel (got shape %s)' % (tuple(weight.shape),))
        self.register_buffer('weight', weight, persistent=False)
        self.ignore_index = ignore_index
        self.label_smoothing = label_smoothing
        self.dice_weight = dice_weight
        self.dice_smooth = dice_smooth
        self.ohem_thresh = ohem_thresh
        self.ohem_min_kept = int(ohem_min_kept)
        self.focal_gamma = focal_gamma
        self.lovasz_weight = lovasz_weight
        self.w = 10.0
        self._triu = {}

    def get_orth_loss(self, proto_sim, is_ft=False):
        # mean |.| over the strict upper triangle, also of a rectangular [K1,K2] matrix (criterion.py:37-43)
        # the reference selects with a boolean mask (a host synchronisation: the element count comes back); the same elements in the same
        # row-major order through constant indices keep the step free of read-backs (HIP-graph capture, graph_step.py) and the sum bit-identical
        if isinstance(proto_sim, OrthTerm):
            return proto_sim.value
        key = (tuple(proto_sim.shape), proto_sim.device)
        idx = self._triu.get(key)
        if idx is None:
            idx = self._triu[key] = torch.triu_indices(proto_sim.shape[0], proto_sim.shape[1], offset=1).to(proto_sim.device)
        return torch.abs(proto_sim[idx[0], idx[1]]).mean()

    def mine(self, preds, target):
        """(mined label map of one head, the kept fraction of its valid pixels) of online hard-pixel mining; nothing here is differentiated"""
        with torch.no_grad():
            mined, _, counts = ops.ohem_mine(preds.detach().float().contiguous(), target, self.ignore_index, self.ohem_thresh, self.ohem_min_kept)
            frac = (counts[2].double() / counts[0].clamp(min=1).double()).float()
        return mined, frac

    def head_loss(self, preds, target):
        """(segmentation loss of one head, its unscaled Dice term or None, its kept fraction or None): head_terms without the Lovasz entry"""
        return self.head_terms(preds, target)[:3]

    def head_terms(self, preds, target):
        """(segmentation loss of one head, its unscaled Dice term or None, its kept fraction or None, its unscaled Lovasz term or None): with dice_weight > 0 one forward
        pass and one backward launch for both terms; with mining on, both run on the head's mined label map; with focal_gamma > 0 the focal forms of the same two
        functions; with lovasz_weight > 0 the same forward passes plus the Lovasz ones and one backward launch for all terms"""
        if self.weight is not None and self.weight.numel() != preds.shape[1]:
            raise ValueError('OrthLoss: %d class weights for %d logit channels' % (self.weight.numel(), preds.shape[1]))
        frac = None
        if self.ohem_thresh is not None:
            target, frac = self.mine(preds, target)
        if self.lovasz_weight > 0.0:
            ce, dice, lov = UpsampleLovaszFn.apply(preds.float(), target.contiguous(), self.ignore_index, self.focal_gamma, self.weight, self.label_smoothing,
                                                   self.dice_weight > 0.0, self.dice_smooth)
            seg = ce if dice is None else torch.add(ce, dice, alpha=self.dice_weight)
            return torch.add(seg, lov, alpha=self.lovasz_weight), dice, frac, lov
        if self.dice_weight > 0.0:
            if self.focal_gamma > 0.0:
                ce, dice = UpsampleFocalDiceFn.apply(preds.float(), target.contiguous(), self.ignore_index, self.focal_gamma, self.weight, self.label_smoothing, self.dice_smooth)
            else:
                ce, dice = UpsampleCEDiceFn.apply(preds.float(), target.contiguous(), self.ignore_index, self.weight, self.label_smoothing, self.dice_smooth)
            return torch.add(ce, dice, alpha=self.dice_weight), dice, frac, None
        if self.focal_gamma > 0.0:
            return UpsampleFocalFn.apply(preds.float(), target.contiguous(), self.ignore_index, self.focal_gamma, self.weight, self.label_smoothing), None, frac, None
        return UpsampleCEFn.apply(preds.float(), target.contiguous(), self.ignore_index, self.weight, self.label_smoothing), None, frac, None

    def seg_loss(self, preds, target):
        return self.head_loss(preds, target)[0]

    def forward(self, preds, target, is_ft=False, proto_sim=None, aux_preds=None):
        seg_loss, dice, frac, lov = self.head_terms(preds, target)
        orth_loss = self.get_orth_loss(proto_sim, is_ft=is_ft)
        if aux_preds is not None:
            aux_loss = self.seg_loss(aux_preds, target)
            total = seg_loss + orth_loss * self.w + 0.4 * aux_loss
            out = {'total_loss': total, 'seg_loss': seg_loss, 'aux_loss': aux_loss, 'orth_loss': orth_loss}
        else:
            # one launch each way (add with alpha; its backward is one scale) instead of mul + add
            out = {'total_loss': torch.add(seg_loss, orth_loss, alpha=self.w), 'seg_loss': seg_loss, 'orth_loss': orth_loss}
        if dice is not None:
            out['dice_loss'] = dice
        if frac is not None:
            out['ohem_frac'] = frac
        if lov is not None:
            out['lovasz_loss'] = lov
        return out
