#!/usr/bin/env python3
"""Same-process A/B of the fused test-time-augmentation kernel (ops.tta_fuse, mode prob, with and without the fused map) against the torch composition of the same formula
on the GPU (per view F.interpolate(align_corners=True), softmax, flip, +=; then / weight sum and argmax).  Seeded random views, three scales each plain and mirrored.  The
versions alternate round by round; every one is warmed up; a repetition is timed with device events; reported: median, min, max and the 10-90 % spread of >= 50
repetitions over >= 0.5 s per version.  The outputs are compared first, with the tolerance of tests/test_tta_gpu.py (float64 evaluation on the GPU as the truth).
usage: tools/tta_fuse_time.py [--classes 12] [--size 1024] [--views 48,64,80] [--batch 1]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from segland_amd import ops
p = argparse.ArgumentParser()
p.add_argument('--classes', type=int, default=12); p.add_argument('--size', type=int, default=1024); p.add_argument('--views', type=str, default='48,64,80')
p.add_argument('--batch', type=int, default=1); p.add_argument('--min-reps', type=int, default=50); p.add_argument('--min-seconds', type=float, default=0.5)
a = p.parse_args()
B, K, H, W = a.batch, a.classes, a.size, a.size
torch.manual_seed(0)
views = []
for s in map(int, a.views.split(',')):
    for flip in (0, 1):
        views.append((torch.randn(B, K, s, s, device='cuda') * 3.0, flip, 1.0))


def torch_composition(vs=views):
    acc, wsum = None, None
    for lg, flip, wt in vs:
        t = torch.softmax(F.interpolate(lg, size=(H, W), mode='bilinear', align_corners=True), dim=1)
        if flip & 1:
            t = t.flip(-1)
        if acc is None:
            acc, wsum = (t * wt if wt != 1.0 else t), wt              # the first term starts the sum (a fresh tensor: no copy)
        else:
            acc.add_(t, alpha=wt); wsum += wt
    acc /= wsum
    return acc.argmax(dim=1), acc


VERSIONS = [('torch composition', torch_composition), ('tta_fuse + map', lambda: ops.tta_fuse(views, (H, W), mode='prob', want_map=True)),
            ('tta_fuse labels only', lambda: ops.tta_fuse(views, (H, W), mode='prob', want_map=False))]

# ---- agreement first: the kernel's error against float64 within max(4 x the float32 composition's own error, 2e-6 x max |fused|); labels equal outside a 1e-5 top-2 margin
lab_t, map_t = torch_composition()
_, map64 = torch_composition([(lg.double(), f, w) for lg, f, w in views])
lab_k, map_k = VERSIONS[1][1]()
lab_n, none = VERSIONS[2][1]()
e_k, e_t, floor = float((map_k.double() - map64).abs().max()), float((map_t.double() - map64).abs().max()), 2e-6 * float(map64.abs().max())
top = map_t.topk(2, dim=1).values
keep = (top[:, 0] - top[:, 1]) >= 1e-5
differ = int((lab_k.long() != lab_t)[keep].sum())
print('B=%d K=%d %dx%d, views %s each plain and mirrored (%d in all), mode prob' % (B, K, H, W, a.views, len(views)))
print('agreement: kernel error %.3g, float32 torch error %.3g vs float64 (floor %.3g); %.4f %% of pixels below the 1e-5 margin, %d labels differ outside it' % (
    e_k, e_t, floor, 100 * (1 - float(keep.float().mean())), differ))
assert e_k <= max(4 * e_t, floor) and differ == 0 and none is None and torch.equal(lab_n, lab_k)
del map64, map_t, map_k, top, keep

# ---- bytes each version moves, from the shapes (float map M = B K H W 4 bytes; the views are read from L2 after the first touch)
M, V, L = B * K * H * W * 4, sum(v[0].numel() * 4 for v in views), B * H * W
nflip = sum(1 for v in views if v[1])
torch_bytes = len(views) * (V // len(views) + M) + len(views) * 2 * M + nflip * 2 * M + (len(views) - 1) * 3 * M + 2 * M + M + 8 * L
print('bytes: torch composition %.0f MB (interpolate w, softmax r+w, flip r+w per mirrored view, += 2r+w per view after the first, / r+w, argmax r + int64 w); tta_fuse + map %.1f MB; labels only %.1f MB'
      % (torch_bytes / 1e6, (V + M + L) / 1e6, (V + L) / 1e6))

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
med = {}
for name, _ in VERSIONS:
    t = sorted(times[name]); n = len(t)
    med[name] = t[n // 2]
    print('%-22s median %8.1f us  min %8.1f  max %8.1f  p10-p90 %8.1f .. %8.1f us  (%d repetitions, %.2f s)' % (
        name, 1e3 * t[n // 2], 1e3 * t[0], 1e3 * t[-1], 1e3 * t[n // 10], 1e3 * t[(9 * n) // 10], n, sum(t) / 1e3))
base = med['torch composition']
for name in ('tta_fuse + map', 'tta_fuse labels only'):
    print('%s: %.2fx the torch composition (%.1f us against %.1f us)' % (name, base / med[name], 1e3 * med[name], 1e3 * base))
print('wall %.1f s' % (time.time() - t0))
