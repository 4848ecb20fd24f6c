#!/usr/bin/env python3
"""Same-process A/B of the fused sliding-window kernel (ops.slide_fuse, with and without the fused map) against the torch composition of the same formula on the GPU
(tests/slide_reference.py: per window F.interpolate(align_corners=True), softmax, times the weight map, += into a [B,K,H,W] accumulator and a weight map; then /, argmax).
Seeded random window logits.  The versions alternate round by round; every one is warmed up; a repetition is timed with device events; reported: median, min, max and the
10-90 % spread of >= 50 repetitions over >= 0.5 s per version.  The outputs are compared first, with the tolerance of tests/test_slide_gpu.py (float64 evaluation on the GPU
as the truth).
usage: tools/slide_fuse_time.py [--classes 12] [--size 1024] [--crop 512] [--stride 341] [--logits 64] [--batch 1] [--mode prob] [--blend uniform]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch
import slide_reference as sr
from eval_common import top2_margin
from segland_amd import ops
p = argparse.ArgumentParser()
p.add_argument('--classes', type=int, default=12); p.add_argument('--size', type=int, default=1024); p.add_argument('--crop', type=int, default=512)
p.add_argument('--stride', type=int, default=341); p.add_argument('--logits', type=int, default=64); p.add_argument('--batch', type=int, default=1)
p.add_argument('--mode', type=str, default='prob'); p.add_argument('--blend', type=str, default='uniform')
p.add_argument('--min-reps', type=int, default=50); p.add_argument('--min-seconds', type=float, default=0.5)
a = p.parse_args()
B, K, H, W = a.batch, a.classes, a.size, a.size
size, crop, stride = (H, W), (a.crop, a.crop), (a.stride, a.stride)
(ch, ys), (cw, xs) = sr.grid(H, crop[0], stride[0]), sr.grid(W, crop[1], stride[1])
N = B * len(ys) * len(xs)
torch.manual_seed(0)
logits = torch.randn(N, K, a.logits, a.logits, device='cuda') * 3.0


def torch_composition(lg=logits):
    return sr.fuse(lg, B, size, crop, stride, a.mode, a.blend)


VERSIONS = [('torch composition', torch_composition), ('slide_fuse + map', lambda: ops.slide_fuse(logits, B, size, crop, stride, mode=a.mode, blend=a.blend, want_map=True)),
            ('slide_fuse labels only', lambda: ops.slide_fuse(logits, B, size, crop, stride, mode=a.mode, blend=a.blend, want_map=False))]

# ---- agreement first: the kernel's error against float64 within max(4 x the float32 composition's own error, 2e-6 x max |fused|); labels equal outside a 1e-5 top-2 margin
lab_t, map_t = torch_composition()
_, map64 = torch_composition(logits.double())
lab_k, map_k = VERSIONS[1][1]()
lab_n, none = VERSIONS[2][1]()
e_k, e_t, floor = float((map_k.double() - map64).abs().max()), float((map_t.double() - map64).abs().max()), 2e-6 * float(map64.abs().max())
keep = top2_margin(map_t) >= 1e-5
differ = int((lab_k.long() != lab_t)[keep].sum())
print('B=%d K=%d scene %dx%d, crop %dx%d, stride %d (offsets %s: %d windows), window logits %dx%d, mode %s, blend %s' % (
    B, K, H, W, ch, cw, a.stride, ','.join(map(str, ys)), N, a.logits, a.logits, a.mode, a.blend))
print('agreement: kernel error %.3g, float32 torch error %.3g vs float64 (floor %.3g); %.4f %% of pixels below the 1e-5 margin, %d labels differ outside it' % (
    e_k, e_t, floor, 100 * (1 - float(keep.float().mean())), differ))
assert e_k <= max(4 * e_t, floor) and differ == 0 and none is None and torch.equal(lab_n, lab_k)
del map64, map_t, map_k, keep

# ---- bytes each version moves, from the shapes (window map Mw = K ch cw 4 bytes, scene map M = B K H W 4 bytes; the window logits are read from L2 after the first touch)
Mw, M, V, L = K * ch * cw * 4, B * K * H * W * 4, logits.numel() * 4, B * H * W
per_window = V // N + Mw + (2 * Mw if a.mode == 'prob' else 0) + 2 * Mw + 3 * Mw       # interpolate r+w, softmax r+w, * weight map r+w, += 2r+w on the window's region
torch_bytes = M + N * per_window + 3 * (len(ys) * len(xs)) * ch * cw * 4 + 2 * M + M + 8 * L
print('bytes: torch composition %.0f MB (accumulator zeroed; per window interpolate w, softmax r+w, * weights r+w, += 2r+w; then / r+w, argmax r + int64 w); slide_fuse + map %.1f MB; '
      'labels only %.1f MB' % (torch_bytes / 1e6, (V + M + L) / 1e6, (V + L) / 1e6))

# ---- timing
for _, fn in VERSIONS:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in VERSIONS}
t0 = time.time()
while min(len(t) for t in times.values()) < a.min_reps or min(sum(t) for t in times.values()) < a.min_seconds * 1e3:
    for name, fn in VERSIONS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1))
        del out
med, spread = {}, {}
for name, _ in VERSIONS:
    t = sorted(times[name]); n = len(t)
    med[name], spread[name] = t[n // 2], t[(9 * n) // 10] - t[n // 10]
    print('%-22s median %8.1f us  min %8.1f  max %8.1f  p10-p90 %8.1f .. %8.1f us  (%d repetitions, %.2f s)' % (
        name, 1e3 * t[n // 2], 1e3 * t[0], 1e3 * t[-1], 1e3 * t[n // 10], 1e3 * t[(9 * n) // 10], n, sum(t) / 1e3))
base = 'torch composition'
for name in ('slide_fuse + map', 'slide_fuse labels only'):
    ahead = med[base] - med[name]
    print('%s: %.2fx the torch composition (%.1f us against %.1f us); the difference %.1f us is %s the two spreads together (%.1f us)' % (
        name, med[base] / med[name], 1e3 * med[name], 1e3 * med[base], 1e3 * ahead, 'above' if ahead > spread[base] + spread[name] else 'NOT above',
        1e3 * (spread[base] + spread[name])))
print('wall %.1f s' % (time.time() - t0))
