#!/usr/bin/env python3
"""Launch times of the POP head and loss kernels by prototype count: Kt = 16 (the kernels for up to 16 prototypes) against Kt = 17, 20, 32 (the wide kernels), at the
bench shape of the head: R = 65 536 rows (B 16, 64 x 64), C = 512, bf16; cross-entropy 64 x 64 -> 512 x 512, tiled and gather backward, with K = Kt + 1 logit channels
-- except in the first row, K = 16: 17 channels already take the wide loss kernels (16 prototypes never ran end to end before them).  Times are of the ops wrappers
(decompose backward and CE forward include their finalize launch)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from segland_amd import _lib, ops

def timeit(fn, it=20):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(it): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3          # us

B, h, C = 16, 64, 512
R, N = B * h * h, h * h
torch.manual_seed(0)
feats = torch.randn(R, C, device='cuda').bfloat16(); dg = torch.randn_like(feats); bg = torch.empty_like(feats)
target = torch.randint(0, 16, (B, 512, 512), device='cuda'); target[:, :40] = 255
one = torch.ones(1, device='cuda')
base = None
print('  Kt   K | decompose fwd    bwd | combine fwd    bwd | CE fwd  bwd tiled  bwd gather   (us; x = ratio to Kt 16)')
for Kt in (16, 17, 20, 32):
    S = F.normalize(torch.randn(Kt, C, device='cuda'), dim=-1)
    proj = ops.pop_decompose_into(feats, S, bg)
    dproj = torch.randn_like(proj); zbg = torch.randn(R, device='cuda'); a = torch.randn(Kt, device='cuda'); b = torch.randn(Kt, device='cuda')
    dpreds = torch.randn(B, 1 + Kt, N, device='cuda')
    K = 16 if Kt == 16 else 1 + Kt
    logits = torch.randn(B, K, h, h, device='cuda')
    out = ops.upsample_ce_fwd(logits, target, 255)
    t = [timeit(lambda: ops.pop_decompose_into(feats, S, bg)), timeit(lambda: ops.pop_decompose_bwd(dg, feats, S, proj, dproj)),
         timeit(lambda: ops.pop_combine_fwd(proj, zbg, a, b, B, N)), timeit(lambda: ops.pop_combine_bwd(dpreds, proj, a, b, B, N)),
         timeit(lambda: ops.upsample_ce_fwd(logits, target, 255)), timeit(lambda: ops.upsample_ce_bwd(logits, target, out, one, 255))]
    _lib.lib().sl_debug_ce_tiled(0)
    t.append(timeit(lambda: ops.upsample_ce_bwd(logits, target, out, one, 255)))
    _lib.lib().sl_debug_reset()
    base = base or t
    print('%4d %3d | ' % (Kt, K) + '  '.join('%7.1f x%4.2f' % (v, v / b0) for v, b0 in zip(t, base)))
