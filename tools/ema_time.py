#!/usr/bin/env python3
"""What the weight EMA costs (profiles/ab_ema.txt).  One GPU, one process, alternating rounds, device events around warmed-up windows.

  (a) the kernel: sl_ema_multi on PSPNet-POP ResNet-50's real parameter list (12 B per element) against sl_adamw_multi on the same list (28 B per element), launched
      through their ops with prebuilt tables (no host work between launches); and the EMA over the whole tracked set (parameters + BatchNorm running statistics).
  (b) the captured training step of bench.py's default configuration (bf16, 16 tiles of 512 x 512, double AdamW step) with and without an attached ModelEma: two models,
      two graphs, windows of replays in turn.

usage: python tools/ema_time.py [--rounds 7] [--calls 30] [--steps 20] [--skip-step]"""
import argparse
import contextlib
import importlib.util
import os
import statistics
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_bench():
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def line(name, xs, unit, extra=''):
    print('  %-44s %9.1f (%9.1f .. %9.1f) %s%s' % (name, statistics.median(xs), min(xs), max(xs), unit, extra))


def make_model(bench, dev, dtype):
    from segland_amd import networks
    from segland_amd.loss.criterion import OrthLoss
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        return networks.pspnet_pop.GFSS_Model(n_base=7, criterion=OrthLoss(255), backbone='resnet50', pretrained_model=None, compute_dtype=dtype, dilated=True, os=8).to(dev).train()


def kernel_part(bench, dev, rounds, calls):
    from segland_amd import ops
    from segland_amd.ema import ModelEma
    model = make_model(bench, dev, torch.bfloat16)
    opt = bench.make_optimizer(model)
    params = [p for g in opt.param_groups for p in g['params']]
    g = torch.Generator().manual_seed(1)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g) * 1e-3).to(dev)
    opt.step(repeat=2)                                           # creates the moments and the device table of the eager launch
    _, adam_table = opt._tables[0]
    n = len(params)
    numel = sum(p.numel() for p in params)
    chunks = sum((p.numel() + 4095) // 4096 for p in params)
    adam = lambda: ops.adamw_multi(adam_table, n, chunks, 0.9, 0.999, 1e-8, 0.5, 0.5, 0.6, 0.6, 2)
    # the EMA over the same list, in the optimizer's order
    shadows = [p.detach().clone() for p in params]
    rec, c = bytearray(), 0
    for s, p in zip(shadows, params):
        rec += struct.pack('<QQqq', s.data_ptr(), p.data_ptr(), p.numel(), c)
        c += (p.numel() + 4095) // 4096
    assert c == chunks
    ema_table = torch.frombuffer(rec, dtype=torch.uint8).to(dev)
    w = torch.tensor([1e-3], dtype=torch.float32, device=dev)
    ema = lambda: ops.ema_multi(ema_table, n, chunks, w)
    full = ModelEma(model, 0.999)
    full_numel = sum(s.numel() for s in full.shadows.values())
    ema_full = lambda: ops.ema_multi(full._table, len(full.names), full._chunks, full._w)
    for fn in (adam, ema, ema_full):
        window_ms(fn, 5)
    t = {'adam': [], 'ema': [], 'full': []}
    for _ in range(rounds):
        t['ema'].append(1e3 * window_ms(ema, calls))
        t['adam'].append(1e3 * window_ms(adam, calls))
        t['full'].append(1e3 * window_ms(ema_full, calls))
    print('(a) PSPNet-POP ResNet-50: %d parameter tensors, %d elements, %d chunks; tracked set with BatchNorm statistics: %d tensors, %d elements' % (
        n, numel, chunks, len(full.names), full_numel))
    print('    us per launch, median (min .. max) of %d alternating rounds of %d launches; GB/s = bytes per element x elements / time' % (rounds, calls))
    line('ema_multi, parameter list (12 B/el)', t['ema'], 'us', '   %7.0f GB/s (%.0f .. %.0f)' % tuple(12e-3 * numel / x for x in (statistics.median(t['ema']), max(t['ema']), min(t['ema']))))
    line('adamw_multi repeat 2, same list (28 B/el)', t['adam'], 'us', '   %7.0f GB/s (%.0f .. %.0f)' % tuple(28e-3 * numel / x for x in (statistics.median(t['adam']), max(t['adam']), min(t['adam']))))
    line('ema_multi, whole tracked set (12 B/el)', t['full'], 'us', '   %7.0f GB/s (%.0f .. %.0f)' % tuple(12e-3 * full_numel / x for x in (statistics.median(t['full']), max(t['full']), min(t['full']))))


def step_part(bench, dev, rounds, steps):
    from segland_amd import graph_step
    from segland_amd.ema import ModelEma
    batches = [bench.synthetic_batch(16, 512, dev, seed=k) for k in range(4)]
    sides = {}
    for name in ('without', 'with'):
        model = make_model(bench, dev, torch.bfloat16)
        opt = bench.make_optimizer(model)
        ema = None
        if name == 'with':
            ema = ModelEma(model, 0.999)
            opt.attach_ema(ema)
        params = [p for p in model.parameters() if p.requires_grad]
        fn = lambda m_, o_, s_, im_, mk_, double_step=True, params=params: (bench.train_step(m_, o_, im_, mk_, params, double_step, 1), None)      # noqa: E731
        for k in range(3):
            bench.train_step(model, opt, *batches[k], params, True, 1)
        graphed = graph_step.GraphedTrainStep(fn, model, opt, None, double_step=True, warmup=0)
        for k in range(3):
            graphed(*batches[k % 4])
        assert graphed.graph is not None, 'the step was not captured'
        sides[name] = (graphed, ema, [0])

    def run(name):
        graphed, _, k = sides[name]
        k[0] += 1
        graphed(*batches[k[0] % 4])
    t = {'without': [], 'with': []}
    for _ in range(rounds):
        for name in ('without', 'with'):
            t[name].append(window_ms(lambda: run(name), steps))
    ema = sides['with'][1]
    assert ema._captured and ema.updates == sides['with'][2][0] + 6, (ema.updates, sides['with'][2][0])
    print('(b) captured training step, bench.py default configuration (PSPNet-POP ResNet-50, bf16, 16 tiles of 512 x 512, double AdamW step): ms per replayed step,')
    print('    median (min .. max) of %d alternating rounds of %d replays; %d EMA updates counted' % (rounds, steps, ema.updates))
    for name in ('without', 'with'):
        print('  %-16s %8.3f (%8.3f .. %8.3f) ms' % (name + ' EMA', statistics.median(t[name]), min(t[name]), max(t[name])))
    print('  difference of the medians %+.3f ms' % (statistics.median(t['with']) - statistics.median(t['without'])))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--calls', type=int, default=30)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--skip-step', action='store_true')
    a = p.parse_args()
    assert torch.cuda.is_available(), 'ema_time.py needs a GPU'
    dev = torch.device('cuda', 0)
    bench = load_bench()
    kernel_part(bench, dev, a.rounds, a.calls)
    torch.cuda.empty_cache()
    if not a.skip_step:
        step_part(bench, dev, a.rounds, a.steps)


if __name__ == '__main__':
    main()
