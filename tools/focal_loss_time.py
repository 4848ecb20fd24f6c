#!/usr/bin/env python3
"""What does the focal modulation cost in the fused upsample + loss kernels, and what does fusing it save?  Device-event times of forward + finalize + backward of

    plain     ops.upsample_ce_fwd / _bwd                              (the yardstick for the cost of the modulation)
    focal     ops.upsample_focal_fwd / _bwd, gamma 2
    torch     F.interpolate(align_corners=True) -> log_softmax -> (1 - p_t)^gamma * nll -> mean over the valid pixels -> autograd   (the yardstick for what fusing saves;
              it materialises the [B, K, 512, 512] logits)

at the bench head shape (B 16, K 8, 64 x 64 -> 512 x 512, rows 0..49 of sample 0 ignored as in bench.py's mask), at K 12 (the fine-tune head) and at K 33 (the widest).
The three are timed in alternating rounds in one process, each round a warmed-up window of LAUNCHES calls ended by a device synchronise; printed: the median over the
rounds in us with (min .. max), the fused pairs also per pass, and the ratios.  Before timing, the focal pair is compared with the torch composition on the same inputs.
A run without a GPU fails."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from segland_amd import ops

B, h, H, ROUNDS, LAUNCHES, GAMMA = 16, 64, 512, 7, 30, 2.0


def timeit(fn, it=LAUNCHES):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(it): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3          # us


def torch_focal(logits, target, gs):
    lg = logits.detach().requires_grad_(True)
    logp = F.interpolate(lg, size=target.shape[1:], mode='bilinear', align_corners=True).log_softmax(1)
    valid = target != 255
    logpt = logp.gather(1, target.masked_fill(~valid, 0)[:, None])[:, 0]
    loss = ((-torch.expm1(logpt)) ** GAMMA * -logpt * valid).sum() / valid.sum()
    (loss * gs).backward()
    return loss.detach(), lg.grad


def main():
    assert torch.cuda.is_available(), 'this tool times GPU kernels: no GPU, no number'
    g = torch.Generator().manual_seed(0)
    one = torch.ones(1, device='cuda')
    fmt = lambda t: '%8.1f (%7.1f .. %7.1f)' % (statistics.median(t), min(t), max(t))
    for K in (8, 12, 33):
        logits = torch.randn(B, K, h, h, generator=g).cuda()
        target = torch.randint(0, K, (B, H, H), generator=g, dtype=torch.int64); target[0, :50] = 255
        target = target.cuda()
        out = ops.upsample_focal_fwd(logits, target, 255, GAMMA)
        dl = ops.upsample_focal_bwd(logits, target, out, one, 255, GAMMA)
        tl, tg = torch_focal(logits, target, one)
        print('K %2d: focal loss %.7g (torch composition %.7g), gradient max abs difference %.3g of max |grad| %.3g'
              % (K, float(out[0]), float(tl), float((dl - tg).abs().max()), float(tg.abs().max())))
        out_p = ops.upsample_ce_fwd(logits, target, 255)
        runs = {
            'plain fwd+finalize': lambda: ops.upsample_ce_fwd(logits, target, 255),
            'plain bwd': lambda: ops.upsample_ce_bwd(logits, target, out_p, one, 255),
            'plain pair': lambda: ops.upsample_ce_bwd(logits, target, ops.upsample_ce_fwd(logits, target, 255), one, 255),
            'focal fwd+finalize': lambda: ops.upsample_focal_fwd(logits, target, 255, GAMMA),
            'focal bwd': lambda: ops.upsample_focal_bwd(logits, target, out, one, 255, GAMMA),
            'focal pair': lambda: ops.upsample_focal_bwd(logits, target, ops.upsample_focal_fwd(logits, target, 255, GAMMA), one, 255, GAMMA),
            'torch composition': lambda: torch_focal(logits, target, one),
        }
        times = {name: [] for name in runs}
        for _ in range(ROUNDS):
            for name, fn in runs.items():
                times[name].append(timeit(fn))
        print('K %2d, B %d, %d x %d -> %d x %d, gamma %g: us per call, median (min .. max) of %d alternating rounds of %d calls' % (K, B, h, h, H, H, GAMMA, ROUNDS, LAUNCHES))
        for name, t in times.items():
            print('  %-20s %s' % (name, fmt(t)))
        med = {name: statistics.median(t) for name, t in times.items()}
        print('  focal / plain: fwd+finalize x%.3f, bwd x%.3f, pair x%.3f;   torch composition / focal pair x%.1f'
              % (med['focal fwd+finalize'] / med['plain fwd+finalize'], med['focal bwd'] / med['plain bwd'], med['focal pair'] / med['plain pair'],
                 med['torch composition'] / med['focal pair']))


if __name__ == '__main__':
    main()
