#!/usr/bin/env python3
"""What does the Lovasz-softmax term cost in the fused upsample + loss path?  Device-event times of

    hist        sl_upsample_lovasz_hist   (zero + histogram pass: one softmax per valid pixel, K LDS increments, then the global integer atomics)
    scan        sl_lovasz_scan            (one block per class + the one-thread sum)
    lovasz fwd  ops.upsample_lovasz_fwd   (both, with the output allocations)
    dice fwd    ops.upsample_ce_dice_fwd  (the yardstick: the hybrid forward + finalize)
    dice bwd    ops.upsample_ce_dice_bwd  (the yardstick for the backward)
    lovasz bwd  ops.upsample_lovasz_bwd   with cross-entropy + Dice + Lovasz in the one launch, and with cross-entropy + Lovasz

at the bench head shape (B 16, K 8, 64 x 64 -> 512 x 512, rows 0..49 of sample 0 ignored as in bench.py's mask), at K 12 (the fine-tune head) and at K 33 (the widest),
on two label / logit pairs: `random` (standard normal logits: the errors spread over all bins) and `trained` (the label's logit raised by 8: most background
errors in the lowest few bins and most foreground errors near them, the hot-address case of a trained model).  Alternating rounds in one process, each a warmed-up window of LAUNCHES
calls ended by a device synchronise; printed: the median over the rounds in us with (min .. max), and the ratios.  A run without a GPU fails."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from segland_amd import _lib, ops
from segland_amd.ops import _p, _s

B, h, H, ROUNDS, LAUNCHES = 16, 64, 512, 7, 30


def timeit(fn, it=LAUNCHES):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(it): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3          # us


def main():
    assert torch.cuda.is_available(), 'this tool times GPU kernels: no GPU, no number'
    L = _lib.lib()
    g = torch.Generator().manual_seed(0)
    fmt = lambda t: '%8.1f (%7.1f .. %7.1f)' % (statistics.median(t), min(t), max(t))
    for K in (8, 12, 33):
        for kind in ('random', 'trained'):
            logits = torch.randn(B, K, h, h, generator=g)
            target = torch.randint(0, K, (B, H, H), generator=g, dtype=torch.int64)
            if kind == 'trained':
                low = target[:, ::H // h, ::H // h]
                logits.scatter_add_(1, low[:, None], torch.full((B, 1, h, h), 8.0))
                target = low.repeat_interleave(H // h, 1).repeat_interleave(H // h, 2).contiguous()
            target[0, :50] = 255
            logits, target = logits.cuda(), target.cuda()
            nbytes = L.sl_lovasz_workspace(K)
            ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
            out2, table = torch.empty(2, device='cuda'), torch.empty(K, L.sl_lovasz_bins(), device='cuda')
            hist = lambda: L.sl_upsample_lovasz_hist(_p(logits), _p(target), B, K, h, h, H, H, 255, _p(ws), nbytes, _s())
            scan = lambda: L.sl_lovasz_scan(_p(ws), K, _p(out2), _p(table), _s())
            assert hist() == 0 and scan() == 0
            lov, table = ops.upsample_lovasz_fwd(logits, target, 255)
            out3, coef = ops.upsample_ce_dice_fwd(logits, target, 255)
            out = ops.upsample_ce_fwd(logits, target, 255)
            gs2, gs3 = torch.ones(2, device='cuda'), torch.ones(3, device='cuda')
            filled = int((ws[:K * table.shape[1] * 8].view(torch.int32) != 0).sum())
            print('K %2d %s: lovasz %.7g over %d present classes, %d of %d bins non-empty' % (K, kind, float(lov[0]), int(lov[1]), filled, K * table.shape[1] * 2))
            runs = {
                'hist': hist, 'scan': scan,
                'lovasz fwd': lambda: ops.upsample_lovasz_fwd(logits, target, 255),
                'dice fwd+finalize': lambda: ops.upsample_ce_dice_fwd(logits, target, 255),
                'plain bwd': lambda: ops.upsample_ce_bwd(logits, target, out, gs2[:1], 255),
                'dice bwd': lambda: ops.upsample_ce_dice_bwd(logits, target, out3, coef, gs2, 255),
                'lovasz bwd ce+dice+lov': lambda: ops.upsample_lovasz_bwd(logits, target, out3, coef, table, gs3, 255),
                'lovasz bwd ce+lov': lambda: ops.upsample_lovasz_bwd(logits, target, out, None, table, gs3, 255),
            }
            times = {name: [] for name in runs}
            for _ in range(ROUNDS):
                for name, fn in runs.items():
                    times[name].append(timeit(fn))
            print('K %2d %s, B %d, %d x %d -> %d x %d: us per call, median (min .. max) of %d alternating rounds of %d calls' % (K, kind, B, h, h, H, H, ROUNDS, LAUNCHES))
            for name, t in times.items():
                print('  %-24s %s' % (name, fmt(t)))
            med = {name: statistics.median(t) for name, t in times.items()}
            print('  hist / dice fwd x%.2f;  lovasz bwd (ce+dice+lov) / dice bwd x%.3f;  lovasz bwd (ce+lov) / plain bwd x%.3f;  the term per head: +%.1f us on the hybrid pair'
                  % (med['hist'] / med['dice fwd+finalize'], med['lovasz bwd ce+dice+lov'] / med['dice bwd'], med['lovasz bwd ce+lov'] / med['plain bwd'],
                     med['lovasz fwd'] + med['lovasz bwd ce+dice+lov'] - med['dice bwd']))


if __name__ == '__main__':
    main()
