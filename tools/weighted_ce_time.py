#!/usr/bin/env python3
"""HIP-event times of the fused upsample + cross-entropy pair with class weights / label smoothing (the weighted kernels) against the plain pair, at the bench shape
(B 16, K 8, 64 x 64 -> 512 x 512) and at the widest head (K 33): forward (with its finalize launch), tiled backward, gather backward.  The variants are timed in
interleaved rounds in one process; the table gives the median over the rounds in us and the ratio to the plain pair."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics
import torch
from segland_amd import _lib, ops

def timeit(fn, it=50):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(it): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3          # us

B, h, H = 16, 64, 512
torch.manual_seed(0)
one = torch.ones(1, device='cuda')
for K in (8, 33):
    logits = torch.randn(B, K, h, h, device='cuda')
    target = torch.randint(0, K, (B, H, H), device='cuda'); target[:, :40] = 255
    w = torch.rand(K, device='cuda') * 1.5 + 0.5
    variants = [('plain', dict()), ('weights', dict(weight=w)), ('smoothing 0.1', dict(label_smoothing=0.1)), ('weights + smoothing 0.1', dict(weight=w, label_smoothing=0.1))]
    times = {name: ([], [], []) for name, _ in variants}
    for _ in range(5):
        for name, kw in variants:
            out = ops.upsample_ce_fwd(logits, target, 255, **kw)
            times[name][0].append(timeit(lambda: ops.upsample_ce_fwd(logits, target, 255, **kw)))
            times[name][1].append(timeit(lambda: ops.upsample_ce_bwd(logits, target, out, one, 255, **kw)))
            _lib.lib().sl_debug_ce_tiled(0)
            times[name][2].append(timeit(lambda: ops.upsample_ce_bwd(logits, target, out, one, 255, **kw)))
            _lib.lib().sl_debug_reset()
    print('K %2d                    |      CE fwd   bwd tiled  bwd gather   (us, median of 5 interleaved rounds; x = ratio to plain)' % K)
    base = [statistics.median(t) for t in times['plain']]
    for name, _ in variants:
        med = [statistics.median(t) for t in times[name]]
        print('%-24s | ' % name + '  '.join('%7.1f x%4.2f' % (v, v / b0) for v, b0 in zip(med, base)))
