#!/usr/bin/env python3
"""HIP-event times of the fused upsample + loss kernels in their three forms -- plain cross-entropy, weighted (class weights + label smoothing 0.1), hybrid (cross-entropy
+ soft Dice, without and with weights) -- at the bench shape (B 16, K 8, 64 x 64 -> 512 x 512) and at the widest head (K 33): forward with its finalize launch, tiled
backward, gather backward (sl_debug_ce_tiled(0)).  The variants are timed in interleaved rounds in one process, 50 launches each after a warm-up; the table gives the
median over the rounds in us and the ratio to the plain pair.  Below it the three passes of online hard-pixel mining (probability, selection, mined map) and their sum through
ops.ohem_mine, in the same interleaved rounds, with the spread of the rounds.  For an A/B of two builds run it alternately with SEGLAND_LIB_PATH at each library."""
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
    # the three passes of online hard-pixel mining in front of those kernels, on logits that are mostly right (+6 at the label of the nearest pixel: the selection then
    # works where the probabilities crowd, just below 1) and on the random ones above; thresh 0.7; min_kept 100000 (the default of the drivers: the threshold decides) and
    # 3500000 (nine tenths of the valid pixels: min_kept decides, q lies in the crowd)
    cell = torch.randint(0, K, (B, h, h), device='cuda')
    blocky = cell.repeat_interleave(H // h, 1).repeat_interleave(H // h, 2).contiguous(); blocky[:, :40] = 255
    right = (logits + 6.0 * torch.nn.functional.one_hot(cell, K).permute(0, 3, 1, 2)).contiguous()
    for what, lg, target, min_kept in (('random logits', logits, target, 100000), ('mostly right', right, blocky, 100000), ('mostly right', right, blocky, 3500000)):
        prob = ops.ohem_prob(lg, target, 255)
        theta, counts = ops.ohem_threshold(prob, 0.7, min_kept)
        mined = torch.empty_like(target)
        passes = [('probability', lambda: ops.ohem_prob(lg, target, 255)), ('selection', lambda: ops.ohem_threshold(prob, 0.7, min_kept)),
                  ('mined map', lambda: _lib.lib().sl_ohem_mine(prob.data_ptr(), target.data_ptr(), theta.data_ptr(), counts.data_ptr(), prob.numel(), 255, mined.data_ptr(), ops._s())),
                  ('all three', lambda: ops.ohem_mine(lg, target, 255, 0.7, min_kept))]
        rounds = {name: [] for name, _ in passes}
        for _ in range(ROUNDS):
            for name, fn in passes:
                rounds[name].append(timeit(fn))
        n, k, kept = counts.tolist()
        print('mining, %s (n %d, k %d, kept %d, theta %.6f) | ' % (what, n, k, kept, float(theta)) + '  '.join(
            '%s %.1f (%.1f .. %.1f) x%.2f' % (name, statistics.median(t), min(t), max(t), statistics.median(t) / base[0]) for name, t in rounds.items())
            + '   (us: median (min .. max) of the rounds; x = ratio to the plain fwd+finalize)')
