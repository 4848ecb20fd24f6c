#!/usr/bin/env python3
"""What --boundary-width costs.  (1) sl_boundary_counts for each band width against sl_confusion_matrix on the same tensors (preallocated outputs, through the C ABI: the
kernels alone): nearest-seed label maps, the prediction's seeds moved by a few pixels, rows 0..49 of every image ignored.  The versions alternate round by round, every
one is warmed up, a round is a window of --calls launches between device events; reported: us per call, median (min .. max) over the rounds, the share of pixels in
the ground-truth band, and the time against the traffic floor (9 B per pixel: the int64 label and the uint8 prediction, each read once, at the 6.29 TB/s a float4 copy
reaches on this chip).  Each width is also timed on maps of ONE label (prediction = target = class 0, nothing ignored): there only the frame of d pixels along the image
edge is band, so nearly no pixel reaches the histogram, and the row is the load and the two passes alone; the difference to the nearest-seed row is what the LDS histogram
costs.  (2) with --forward: one 1024 x 1024 tile the way eval_base scores it at its default batch of 1 -- the bf16 eval-mode forward of PSPNet-POP resnet50 (random
weights: the time does not depend on them) + the fused upsample + argmax -- beside ops.boundary_counts on one tile, device events around single calls: the cost of the
flag against the forward pass that made the map.  (3) with --eval: wall time of eval_base on the synthetic set (128 x 128 tiles) with the flag off and on, alternating,
after one warm-up run of each.
usage: tools/boundary_time.py [--batch 16] [--size 1024] [--classes 12] [--widths 3,29] [--seeds 40] [--calls 20] [--rounds 15] [--forward] [--eval]
  --batch, --size, --classes   the label maps of (1): B x size x size, K classes        --widths   band widths d to time, comma-separated
  --seeds   seed points per image of the nearest-seed maps                               --calls    launches per timed window        --rounds   alternating rounds
  --forward, --eval   add section (2) / section (3)"""
import argparse, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch
from segland_amd import _lib, ops
p = argparse.ArgumentParser()
p.add_argument('--batch', type=int, default=16); p.add_argument('--size', type=int, default=1024); p.add_argument('--classes', type=int, default=12)
p.add_argument('--widths', type=str, default='3,29'); p.add_argument('--seeds', type=int, default=40); p.add_argument('--calls', type=int, default=20)
p.add_argument('--rounds', type=int, default=15); p.add_argument('--eval', action='store_true'); p.add_argument('--forward', action='store_true')
a = p.parse_args()
B, H, W, K = a.batch, a.size, a.size, a.classes
widths = [int(v) for v in a.widths.split(',')]
HBM = 6.29e12


def voronoi(seeds, classes):
    y, x = torch.meshgrid(torch.arange(H, device='cuda', dtype=torch.float32), torch.arange(W, device='cuda', dtype=torch.float32), indexing='ij')
    best = torch.full((H, W), float('inf'), device='cuda'); lab = torch.zeros((H, W), dtype=torch.int64, device='cuda')
    for (sy, sx), c in zip(seeds.tolist(), classes.tolist()):
        dist = (y - sy) ** 2 + (x - sx) ** 2
        lab = torch.where(dist < best, torch.full_like(lab, c), lab); best = torch.minimum(best, dist)
    return lab


torch.manual_seed(0)
target = torch.empty((B, H, W), dtype=torch.int64, device='cuda'); pred = torch.empty((B, H, W), dtype=torch.uint8, device='cuda')
for b in range(B):
    seeds, classes = torch.rand(a.seeds, 2) * torch.tensor([H, W]), torch.randint(0, K, (a.seeds,))
    target[b] = voronoi(seeds, classes); pred[b] = voronoi(seeds + torch.tensor([3.0, -2.0]), classes).to(torch.uint8)
target[:, :50] = 255
L = _lib.lib()
cm = torch.zeros((K, K), dtype=torch.int64, device='cuda'); counts = torch.zeros((3, K), dtype=torch.int64, device='cuda'); band_cm = torch.zeros_like(cm)
stream = torch.cuda.current_stream().cuda_stream


def confusion():
    ops.check(L.sl_confusion_matrix(pred.data_ptr(), target.data_ptr(), target.numel(), K, 255, cm.data_ptr(), stream), 'confusion_matrix')


flat_t, flat_p = torch.zeros_like(target), torch.zeros_like(pred)     # one label everywhere: only the frame along the image edge is band


def boundary(d, p=pred, t=target):
    return lambda: ops.check(L.sl_boundary_counts(p.data_ptr(), t.data_ptr(), B, H, W, K, 255, d, counts.data_ptr(), band_cm.data_ptr(), stream), 'boundary_counts')


VERSIONS = ([('confusion_matrix', confusion)] + [('boundary_counts d=%d' % d, boundary(d)) for d in widths]
            + [('boundary_counts d=%d, one label' % d, boundary(d, flat_p, flat_t)) for d in widths])
print('B=%d %dx%d, K=%d, %d seeds per image, rows 0..49 ignored; windows of %d calls, %d alternating rounds' % (B, H, W, K, a.seeds, a.calls, a.rounds))
for d in widths:
    c, m = ops.boundary_counts(pred, target, K, 255, d)
    full = ops.confusion_matrix(pred, target, K, 255)
    assert bool((m <= full).all()) and torch.equal(m.sum(1), c[1]) and bool((c[0] <= torch.minimum(c[1], c[2])).all())
    print('d=%d: %.2f %% of the scored pixels in the ground-truth band, %.2f %% in the prediction band; boundary IoU (all classes pooled) %.4f, full-map pixel accuracy %.4f' % (
        d, 100.0 * float(c[1].sum()) / float(full.sum()), 100.0 * float(c[2].sum()) / float(full.sum()), float(c[0].sum()) / float(c[1].sum() + c[2].sum() - c[0].sum()),
        float(full.diag().sum()) / float(full.sum())))
for _, fn in VERSIONS:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in VERSIONS}
for _ in range(a.rounds):
    for name, fn in VERSIONS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record(); torch.cuda.synchronize()
        times[name].append(1e3 * e0.elapsed_time(e1) / a.calls)
floor = 9.0 * B * H * W / HBM * 1e6
med = {}
for name, _ in VERSIONS:
    t = sorted(times[name]); med[name] = t[len(t) // 2]
    print('  %-34s %8.1f us per call (%8.1f .. %8.1f)   %.2fx the %.1f us traffic floor (9 B per pixel at 6.29 TB/s)' % (name, med[name], t[0], t[-1], med[name] / floor, floor))
for d in widths:
    full, flat = med['boundary_counts d=%d' % d], med['boundary_counts d=%d, one label' % d]
    print('  boundary_counts d=%d / confusion_matrix x%.2f;  load + passes (one label) %.1f us = %.0f %% of it, the histogram of the band pixels the other %.1f us' % (
        d, full / med['confusion_matrix'], flat, 100.0 * flat / full, full - flat))

if a.forward:
    # the forward pass that makes the map the kernel scores: one 1024 x 1024 tile (eval's default batch), bf16, eval mode, + the fused upsample + argmax
    from segland_amd.networks.pspnet_pop import GFSS_Model
    model = GFSS_Model(n_base=7, backbone='resnet50', dilated=True, os=8, n_novel=4, is_ft=False, pretrained_model=None).to('cuda').eval()
    image = torch.randn(1, 3, H, W, device='cuda')

    def forward():
        with torch.no_grad():
            return ops.upsample_argmax(model(image).float().contiguous(), (H, W))
    one = [('forward + argmax, 1 tile', forward)] + [('boundary_counts d=%d, 1 tile' % d, (lambda d: lambda: ops.boundary_counts(pred[:1], target[:1], K, 255, d))(d)) for d in widths]
    for name, fn in one:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        ts.sort()
        print('  %-32s %9.1f us per call (%9.1f .. %9.1f), op wrapper and its allocations included' % (name, ts[5], ts[0], ts[-1]))

if a.eval:
    from eval_common import EVAL_ARGS
    from segland_amd import eval_base

    def run(extra):
        with tempfile.TemporaryDirectory() as out:
            torch.manual_seed(0); torch.cuda.synchronize(); t0 = time.time()
            eval_base.main(EVAL_ARGS + ['--save-path', out] + extra)
            torch.cuda.synchronize()
            return time.time() - t0
    flags = {'off': [], 'on (d=3)': ['--boundary-width', '3']}
    wall = {k: [] for k in flags}
    for i in range(4):
        for k, extra in flags.items():
            t = run(extra)
            if i:
                wall[k].append(t)                                    # round 0 warms both up
    print('eval_base on the synthetic set (128 x 128 tiles, resnet50, random weights), wall seconds of 3 alternating runs after a warm-up:')
    for k in flags:
        print('  --boundary-width %-9s %s   median %.3f s' % (k, ' '.join('%.3f' % t for t in wall[k]), sorted(wall[k])[1]))
