#!/usr/bin/env python3
"""Same-process A/B of the three tile preparation entries (csrc/augment.hip) on HBM-resident raw tiles: sl_augment_batch, sl_augment_batch_ex at the identity rescale (the
yardstick), and sl_augment_batch_geo with rotate = blur_k = 0 (same output as the former two, bit for bit -- checked first), with a rotation only, with a 5-tap blur only, and
with rotation + 11-tap blur + colour jitter.  The device tables are built once; a repetition is ONE launch, timed with device events; the versions alternate round by round,
every one warmed up with 5 launches; reported: median, min, max and the 10-90 % spread of >= 50 repetitions over >= 0.5 s per version.
usage: tools/aug_geo_time.py [--batch 16] [--tile 1024] [--crop 512]"""
import argparse, math, os, struct, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from segland_amd import _lib
from segland_amd.dataset.augment import GeoDraw, TileAugmenter
from segland_amd.ops import _p, _s
p = argparse.ArgumentParser()
p.add_argument('--batch', type=int, default=16); p.add_argument('--tile', type=int, default=1024); p.add_argument('--crop', type=int, default=512)
p.add_argument('--min-reps', type=int, default=50); p.add_argument('--min-seconds', type=float, default=0.5)
a = p.parse_args()
B, T, Cr = a.batch, a.tile, a.crop
dev = torch.device('cuda', 0)
g = torch.Generator().manual_seed(0)
imgs = [torch.randint(0, 256, (T, T, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
lbls = [torch.randint(0, 12, (T, T), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
aug = TileAugmenter((Cr, Cr), device=dev)
lib = _lib.lib()
rng = np.random.RandomState(0)
out, lab = torch.empty((B, 3, Cr, Cr), device=dev), torch.empty((B, Cr, Cr), dtype=torch.int64, device=dev)
offs = [(int(rng.randint(0, T - Cr + 1)), int(rng.randint(0, T - Cr + 1))) for _ in range(B)]
angles = [float(rng.uniform(-180.0, 180.0)) for _ in range(B)]


def table(rotate, blur_k, jitter, geo=True):
    rec = b''
    for b in range(B):
        t = math.radians(angles[b])
        d = GeoDraw(offs[b][0], offs[b][1], b % 2, b % 4, T, T, int(jitter), 1.0 + 0.3 * (b % 3 - 1), 0.1 * (b % 5 - 2), 1.0 + 0.2 * (b % 4 - 1.5), T, 0,
                    int(rotate), math.cos(t) if rotate else 1.0, math.sin(t) if rotate else 0.0, blur_k)
        rec += aug._record_ex(imgs[b].data_ptr(), lbls[b].data_ptr(), T, T, d, geo)
    return torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(dev)


rec, flags = b'', []
for b in range(B):
    rec += struct.pack('<QQiiii', imgs[b].data_ptr(), lbls[b].data_ptr(), T, T, offs[b][0], offs[b][1])
    flags += [b % 2, b % 4]
plain_table, plain_flags = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(dev), torch.tensor(flags, dtype=torch.int32).to(dev)
ex_table = table(False, 0, False, geo=False)
tables = {'geo identity': table(False, 0, False), 'geo rotation': table(True, 0, False), 'geo blur 5': table(False, 5, False), 'geo rotation + blur 11 + jitter': table(True, 11, True)}


def plain():
    _lib.check(lib.sl_augment_batch(_p(plain_table), _p(plain_flags), B, Cr, Cr, aug.mean, aug.std, 255, None, _p(out), _p(lab), _s()), 'augment_batch')


def ex():
    _lib.check(lib.sl_augment_batch_ex(_p(ex_table), B, Cr, Cr, aug.mean, aug.std, 255, None, _p(out), _p(lab), _s()), 'augment_batch_ex')


def geo(name):
    return lambda: _lib.check(lib.sl_augment_batch_geo(_p(tables[name]), B, Cr, Cr, aug.mean, aug.std, 255, None, _p(out), _p(lab), _s()), 'augment_batch_geo')


VERSIONS = [('sl_augment_batch', plain), ('ex scale 1.0', ex)] + [(n, geo(n)) for n in tables]
plain(); want = (out.clone(), lab.clone())
for _, fn in VERSIONS[1:3]:
    out.zero_(); fn()
    assert torch.equal(out, want[0]) and torch.equal(lab, want[1]), 'the identity record differs from sl_augment_batch'
print('B=%d, %dx%d uint8 tiles resident in HBM -> %dx%d crops; every launch writes %.1f MB (float image + int64 label); ex and geo at the identity == sl_augment_batch bit for bit' % (
    B, T, T, Cr, Cr, (out.numel() * 4 + lab.numel() * 8) / 1e6))
for _, fn in VERSIONS:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in VERSIONS}
t0 = time.time()
while min(len(t) for t in times.values()) < a.min_reps or min(sum(t) for t in times.values()) < a.min_seconds * 1e3:
    for name, fn in VERSIONS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1))
    if time.time() - t0 > 60:
        break
med = {}
for name, _ in VERSIONS:
    t = sorted(times[name]); n = len(t)
    med[name] = t[n // 2]
    print('%-32s median %8.1f us  min %8.1f  max %8.1f  p10-p90 %8.1f .. %8.1f us  (%d repetitions, %.2f s)' % (
        name, 1e3 * t[n // 2], 1e3 * t[0], 1e3 * t[-1], 1e3 * t[n // 10], 1e3 * t[(9 * n) // 10], n, sum(t) / 1e3))
for name in tables:
    print('%s: %.2fx ex scale 1.0 (%.1f us against %.1f us)' % (name, med[name] / med['ex scale 1.0'], 1e3 * med[name], 1e3 * med['ex scale 1.0']))
print('wall %.1f s' % (time.time() - t0))
