#!/usr/bin/env python3
"""HIP-event times of the fused upsample + loss kernels in their three forms -- plain cross-entropy, weighted (class weights + label smoothing 0.1), hybrid (cross-entropy
+ soft Dice, without and with weights) -- at the bench shape (B 16, K 8, 64 x 64 -> 512 x 512) and at the widest head (K 33): forward with its finalize launch, tiled
backward, gather backward (sl_debug_ce_tiled(0)).  The variants are timed in interleaved rounds in one process, 50 launches each after a warm-up; the table gives the
median over the rounds in us and the ratio to the plain pair.  For an A/B of two builds run it alternately with SEGLAND_LIB_PATH at each library."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from segland_amd import _lib, ops


def timeit(fn, it=50):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(it): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3          # us


B, h, H, ROUNDS = 16, 64, 512, 5
torch.manual_seed(0)
one, two = torch.ones(1, device='cuda'), torch.tensor([1.0, 0.5], device='cuda')
for K in (8, 33):
    logits = torch.randn(B, K, h, h, device='cuda')
    target = torch.randint(0, K, (B, H, H), device='cuda'); target[:, :40] = 255
    w = torch.rand(K, device='cuda') * 1.5 + 0.5
    variants = [('plain', False, dict()), ('weighted', False, dict(weight=w, label_smoothing=0.1)),
                ('hybrid', True, dict()), ('hybrid weighted', True, dict(weight=w, label_smoothing=0.1))]
    times = {name: ([], [], []) for name, _, _ in variants}
    for _ in range(ROUNDS):
        for name, dice, kw in variants:
            if dice:
                out, coef = ops.upsample_ce_dice_fwd(logits, target, 255, **kw)
                fwd = lambda: ops.upsample_ce_dice_fwd(logits, target, 255, **kw)
                bwd = lambda: ops.upsample_ce_dice_bwd(logits, target, out, coef, two, 255, **kw)
            else:
                out = ops.upsample_ce_fwd(logits, target, 255, **kw)
                fwd = lambda: ops.upsample_ce_fwd(logits, target, 255, **kw)
                bwd = lambda: ops.upsample_ce_bwd(logits, target, out, one, 255, **kw)
            times[name][0].append(timeit(fwd))
            times[name][1].append(timeit(bwd))
            _lib.lib().sl_debug_ce_tiled(0)
            times[name][2].append(timeit(bwd))
            _lib.lib().sl_debug_reset()
    print('K %2d             |  fwd+finalize   bwd tiled  bwd gather   (us, median of %d interleaved rounds of 50 launches; x = ratio to plain)' % (K, ROUNDS))
    base = [statistics.median(t) for t in times['plain']]
    for name, _, _ in variants:
        med = [statistics.median(t) for t in times[name]]
        print('%-16s | ' % name + '  '.join('%7.1f x%4.2f' % (v, v / b0) for v, b0 in zip(med, base)))
