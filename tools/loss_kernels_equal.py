#!/usr/bin/env python3
"""Do two builds of the library compute the same bits in the fused upsample + loss kernels?  Forward + finalize + backward through segland_amd.ops over every form
(plain, weights, smoothing, both, hybrid plain, hybrid weights + smoothing), both backward routes (tiled; gather through sl_debug_ce_tiled(0)) and the shapes of the
GPU tests (every KW instantiation, the one-pass and the channel-sliced tiled kernel, a ragged last tile, scale 1).  Inputs come from CPU generators with fixed seeds;
some labels are ignored and some lie outside [0, K).  One line per case with the sha1 of the loss vector, the coefficient table and dlogits:

    SEGLAND_LIB_PATH=/path/to/parent/libsegland_hip.so python tools/loss_kernels_equal.py > a.txt
    python tools/loss_kernels_equal.py > b.txt && cmp a.txt b.txt"""
import hashlib
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from segland_amd import _lib, ops

SHAPES = [(8, (8, 8), (64, 64)), (12, (9, 7), (40, 33)), (21, (9, 7), (40, 33)), (33, (8, 8), (64, 64)), (33, (8, 8), (8, 8)), (17, (5, 6), (64, 64))]
FORMS = [('plain', False, False, 0.0), ('weights', False, True, 0.0), ('smoothing', False, False, 0.1), ('weights+smoothing', False, True, 0.1),
         ('hybrid plain', True, False, 0.0), ('hybrid weights+smoothing', True, True, 0.1)]
B, IGNORE = 3, 255


def sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def main():
    L = _lib.lib()
    two = torch.tensor([0.75, 0.5], device='cuda')
    for si, (K, (h, w), (H, W)) in enumerate(SHAPES):
        g = torch.Generator(device='cpu').manual_seed(100 + si)
        logits = (torch.randn(B, K, h, w, generator=g) * 2.0).cuda()
        target = torch.randint(0, K, (B, H, W), generator=g)
        mark = torch.rand(B, H, W, generator=g)
        target[mark < 0.10] = IGNORE
        target[(mark >= 0.10) & (mark < 0.13)] = K + 2          # outside [0, K): counts as ignored
        target[(mark >= 0.13) & (mark < 0.15)] = -1
        target = target.cuda()
        weight = (torch.rand(K, generator=g) * 1.5 + 0.5).cuda()
        for name, dice, wt, eps in FORMS:
            kw = dict(weight=weight if wt else None, label_smoothing=eps)
            for route in ('tiled', 'gather'):
                if route == 'gather':
                    L.sl_debug_ce_tiled(0)
                try:
                    if dice:
                        out, coef = ops.upsample_ce_dice_fwd(logits, target, IGNORE, **kw)
                        dl = ops.upsample_ce_dice_bwd(logits, target, out, coef, two, IGNORE, **kw)
                    else:
                        out, coef = ops.upsample_ce_fwd(logits, target, IGNORE, **kw), None
                        dl = ops.upsample_ce_bwd(logits, target, out, two[:1], IGNORE, **kw)
                    torch.cuda.synchronize()
                finally:
                    L.sl_debug_reset()
                assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dl).all()), (name, route, K)
                print('K %2d %s -> %s %-24s %-6s loss %s coef %s dlogits %s' % (K, (h, w), (H, W), name, route, sha(out), sha(coef) if dice else '-' * 16, sha(dl)))


if __name__ == '__main__':
    main()
