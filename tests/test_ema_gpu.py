"""Weight EMA (--ema-decay) on the GPU: the multi-tensor kernel sl_ema_multi against the float64 recurrence (odd sizes, chunk edges, views at 4- and 8-byte offsets,
sentinels around every tensor), its two exact invariants, the table lookup and the grid-stride loop past the grid cap; the optimizer hook of segland_amd.optim.AdamW /
SGD (the step itself unchanged bit for bit); the captured training and fine-tune steps against the kernel-by-kernel loop (shadows and update counts bit-identical, the
model and the losses bit-identical to a run WITHOUT an EMA); applied() against a deep copy loaded from model_state_dict(), with the caches invalidated in both
directions; and both drivers end to end with --ema-decay, including a -c resume.  Without the feature every test here fails (missing symbol, attribute or flag).

The error bound of every comparison with the float64 recurrence e <- e + (s - e) w:  |err| <= 4 T 2^-24 M  after T updates, M = max(|src|, |ema|) over the run: a step
rounds at most three times (the difference, the product, the sum) on magnitudes <= 2M, each by at most 2^-24 of it, and carries the earlier error with the factor
1 - w < 1."""
import copy
import glob
import os
import struct

import numpy as np
import pytest
import torch

from oracle import formula as fm

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -12345.678


def _w(t, decay=0.9, warmup=True):
    return float(np.float32(1.0 - (min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay)))


def _table(pairs):
    """device table of sl_ema_multi for [(ema view, src view)] -> (table, n, total_chunks)"""
    rec, chunks = bytearray(), 0
    for e, s in pairs:
        assert e.is_contiguous() and s.is_contiguous() and e.numel() == s.numel() and e.dtype == s.dtype == torch.float32
        rec += struct.pack('<QQqq', e.data_ptr(), s.data_ptr(), e.numel(), chunks)
        chunks += (e.numel() + 4095) // 4096
    return torch.frombuffer(rec, dtype=torch.uint8).to(DEV), len(pairs), chunks


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(table, n, chunks, w):
    from segland_amd import ops
    wd = torch.tensor([w], dtype=torch.float32, device=DEV)
    ops.ema_multi(table, n, chunks, wd)
    return wd


def _layout():
    """Two flat buffers (ema, src) with the eight tensors of the issue at chosen misalignments and sentinel gaps of at least one element between them, plus three pairs
    of views into aligned bases: ema at +4 bytes / src aligned, ema aligned / src at +8 bytes, both at +4 bytes."""
    sizes = [1, 3, 4, 5, 4095, 4096, 4097, 12293]
    shifts = [0, 0, 0, 1, 3, 0, 2, 0]                      # element offset past a 16-byte boundary
    offs, pos = [], 0
    for n, sh in zip(sizes, shifts):
        pos = (pos + 1 + 3) // 4 * 4 + sh                  # at least one sentinel in front
        offs.append(pos)
        pos += n
    total = pos + 5
    g = torch.Generator().manual_seed(11)
    ema_flat = (torch.randn(total, generator=g) * 2).to(DEV)
    src_flat = torch.empty(total, device=DEV)
    mask = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        mask[o:o + n] = False
    mask = mask.to(DEV)
    ema_flat[mask] = SENTINEL
    pairs = [(ema_flat[o:o + n], src_flat[o:o + n]) for o, n in zip(offs, sizes)]
    assert ema_flat.data_ptr() % 16 == 0 and src_flat.data_ptr() % 16 == 0
    bases = [torch.full((4200,), SENTINEL, device=DEV) for _ in range(6)]
    views = [(bases[0][1:1 + 4100], bases[1][0:4100]), (bases[2][0:4103], bases[3][2:2 + 4103]), (bases[4][1:1 + 4098], bases[5][1:1 + 4098])]
    for e, s in views:
        e.copy_(torch.randn(e.numel(), generator=g))
    return ema_flat, src_flat, mask, pairs, bases, views


def test_kernel_against_the_float64_recurrence(hip):
    ema_flat, src_flat, mask, pairs, bases, views = _layout()
    recs = pairs + views
    aligned = [(e.data_ptr() | s.data_ptr()) % 16 == 0 for e, s in recs]
    assert any(a and e.numel() > 4096 for a, (e, _) in zip(aligned, recs)) and any(not a and e.numel() > 4096 for a, (e, _) in zip(aligned, recs))
    table, n, chunks = _table(recs)
    ref = [e.double().clone() for e, _ in recs]
    g = torch.Generator().manual_seed(12)
    T, M = 5, max(float(e.abs().max()) for e, _ in recs)
    for t in range(T):
        src_flat.copy_(torch.randn(src_flat.numel(), generator=g) * 3)
        src_flat[mask] = SENTINEL
        for k in (1, 3, 5):
            bases[k].fill_(SENTINEL)
        for _, s in views:
            s.copy_(torch.randn(s.numel(), generator=g) * 3)
        src_before = [_bits(src_flat).clone()] + [_bits(bases[k]).clone() for k in (1, 3, 5)]
        w = _w(t)
        _launch(table, n, chunks, w)
        for r, (e, s) in zip(ref, recs):
            M = max(M, float(s.abs().max()), float(r.abs().max()))
            r += (s.double() - r) * w
        for before, now in zip(src_before, [src_flat] + [bases[k] for k in (1, 3, 5)]):
            assert torch.equal(before, _bits(now)), 'a source was written'
    worst = max(float((e.double() - r).abs().max()) for r, (e, _) in zip(ref, recs))
    bound = 4 * T * 2.0 ** -24 * M
    print('ema_multi vs float64 recurrence after %d updates: max |err| %.3g, bound %.3g (M %.3g)' % (T, worst, bound, M))
    assert worst <= bound
    sent = _bits(torch.tensor([SENTINEL], device=DEV))[0]
    assert bool((_bits(ema_flat)[mask] == sent).all()) and bool((_bits(src_flat)[mask] == sent).all()), 'a sentinel next to a tensor was written'
    for k, (lo, hi) in zip((0, 2, 4), ((1, 4101), (0, 4103), (1, 4099))):
        keep = torch.ones(4200, dtype=torch.bool, device=DEV)
        keep[lo:hi] = False
        assert bool((_bits(bases[k])[keep] == sent).all()), 'a sentinel around view %d was written' % k


def test_exact_invariants(hip):
    """w == 0 keeps the bits of ema (negative zero and denormals included), src == ema keeps them for any w, and two runs from the same state give the same bits"""
    ema_flat, src_flat, mask, pairs, bases, views = _layout()
    recs = pairs + views
    table, n, chunks = _table(recs)
    g = torch.Generator().manual_seed(13)
    src_flat.copy_(torch.randn(src_flat.numel(), generator=g))
    for _, s in views:
        s.copy_(torch.randn(s.numel(), generator=g))
    special = torch.tensor([-0.0, 0.0, 1e-40, -1e-40, 1.17549435e-38, 65504.0, -1e30, 3.0], device=DEV)
    pairs[7][0][:8] = special
    pairs[6][0][:8] = special                                    # a misaligned tensor too: the scalar path
    state = [e.clone() for e, _ in recs]
    _launch(table, n, chunks, 0.0)
    for (e, _), before in zip(recs, state):
        assert torch.equal(_bits(e), _bits(before)), 'w == 0 changed an average'
    for e, s in recs:
        s.copy_(e)
    for w in (0.1, 1.0, _w(3)):
        _launch(table, n, chunks, w)
        for (e, _), before in zip(recs, state):
            assert torch.equal(_bits(e), _bits(before)), 'src == ema changed an average (w %g)' % w
    for _, s in recs:
        s.copy_(torch.randn(s.numel(), generator=g))
    _launch(table, n, chunks, 0.25)
    first = [e.clone() for e, _ in recs]
    assert any(not torch.equal(a, b) for a, b in zip(first, state))
    for (e, _), before in zip(recs, state):
        e.copy_(before)
    _launch(table, n, chunks, 0.25)
    for (e, _), a in zip(recs, first):
        assert torch.equal(_bits(e), _bits(a)), 'two runs differ'


@pytest.mark.parametrize('ones,big', [(300, 3 * 4096 + 1), (8200, 2 * 4096 + 5)])
def test_lookup_and_grid_stride(hip, ones, big):
    """Many one-element records (a chunk each) in front of a large one: the binary search over the table, and -- 8203 chunks against the launcher's cap of 8192 blocks --
    the grid-stride loop"""
    g = torch.Generator().manual_seed(14)
    ema = torch.randn(ones + big + 8, generator=g).to(DEV)
    src = torch.randn(ones + big + 8, generator=g).to(DEV)
    recs = [(ema[i:i + 1], src[i:i + 1]) for i in range(ones)] + [(ema[ones:ones + big], src[ones:ones + big])]
    table, n, chunks = _table(recs)
    assert n == ones + 1 and chunks == ones + (big + 4095) // 4096 and (ones < 8192) == (chunks < 8192)
    before, w = ema.clone(), _w(2)
    _launch(table, n, chunks, w)
    want = before.double() + (src.double() - before.double()) * w
    M = max(float(before.abs().max()), float(src.abs().max()))
    worst = float((ema.double() - want)[:ones + big].abs().max())
    print('%d records, %d chunks: max |err| %.3g, bound %.3g' % (n, chunks, worst, 4 * 2.0 ** -24 * M))
    assert worst <= 4 * 2.0 ** -24 * M                                                   # an element that was not visited misses it by orders of magnitude
    assert torch.equal(_bits(ema[ones + big:]), _bits(before[ones + big:]))            # nothing behind the last record


# --------------------------------------------------------------------------------------------- optimizer hook, eager
class _Params(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(21)
        self.p = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((7,), (64, 33), (4097,), (3, 5, 2))])


@pytest.mark.parametrize('kind,repeat', [('adamw', 1), ('adamw', 2), ('sgd', 1)])
def test_optimizer_hook_eager(hip, kind, repeat):
    """4 steps: parameters and optimizer state bit-identical to the same optimizer with no EMA attached; one EMA update per step() call (also for the folded double
    step); shadows within the bound of the recurrence over the parameters read back after each step"""
    from segland_amd.ema import ModelEma
    from segland_amd.optim import SGD, AdamW

    def run(with_ema):
        m = _Params().to(DEV)
        opt = AdamW(m.parameters(), lr=1e-2, weight_decay=1e-2) if kind == 'adamw' else SGD(m.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
        ema = None
        if with_ema:
            ema = ModelEma(m, 0.9)
            opt.attach_ema(ema)
            assert ema._table is not None, 'the kernel path was not taken'
        ref = {k: s.double().clone() for k, s in ema.shadows.items()} if with_ema else None
        g, M = torch.Generator().manual_seed(22), 0.0
        for t in range(4):
            for p in m.parameters():
                p.grad = torch.randn(p.shape, generator=g).to(DEV)
            if kind == 'adamw':
                opt.step(repeat=repeat)
            else:
                opt.step()
            if with_ema:
                assert ema.updates == t + 1
                live = m.state_dict()
                for k in ref:
                    M = max(M, float(live[k].abs().max()), float(ref[k].abs().max()))
                    ref[k] += (live[k].double() - ref[k]) * _w(t)
        return m, opt, ema, ref, M

    m0, o0, _, _, _ = run(False)
    m1, o1, ema, ref, M = run(True)
    for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
        assert torch.equal(a, b), k
    for s0, s1 in zip(o0.state.values(), o1.state.values()):
        assert s0.keys() == s1.keys()
        for k in s0:
            assert torch.equal(torch.as_tensor(s0[k]), torch.as_tensor(s1[k])), k
    worst = max(float((ema.shadows[k].double() - ref[k]).abs().max()) for k in ref)
    bound = 4 * 4 * 2.0 ** -24 * M
    print('%s repeat %d: shadows vs recurrence max |err| %.3g, bound %.3g' % (kind, repeat, worst, bound))
    assert len(ref) == 4 and worst <= bound
    assert all(not torch.equal(ema.shadows[k], m1.state_dict()[k]) for k in ref)


# --------------------------------------------------------------------------------------------- captured steps (the _run pattern of test_graph_step_gpu.py)
def _pspnet(dtype):
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.networks.pspnet_pop import GFSS_Model
    m = GFSS_Model(n_base=7, criterion=OrthLoss(255), backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=dtype)
    fm.load_formula_weights(m)
    return m.to(DEV).train()


def _batches(n, B, H, W):
    out = []
    for k in range(n):
        img = fm.formula_image(B, H, W, 'gs/img%d' % k).to(DEV)
        mask = fm.formula_mask(B, H, W, 8, 'gs/mask%d' % k, block=16, ignore_rows=4).to(DEV)
        out.append((img, mask))
    return out


def _run(model, batches, graphed, with_ema, odd=None, lr=1e-4):
    from segland_amd import graph_step
    from segland_amd.ema import ModelEma
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    opt = AdamW(get_parameters(model, lr=lr), lr=lr, weight_decay=1e-4)
    ema = None
    if with_ema:
        ema = ModelEma(model, 0.9)
        opt.attach_ema(ema)
    scaler = NativeScalerWithGradNormCount()
    step = graph_step.GraphedTrainStep(train_iteration, model, opt, scaler, double_step=True, warmup=2) if graphed else None
    log = []
    for k, (img, mask) in enumerate(batches):
        if odd is not None and k == odd[0]:                      # a batch of another shape: runs eagerly, the graph survives it
            d, gn = (step(*odd[1]) if graphed else train_iteration(model, opt, scaler, *odd[1], double_step=True))
            log.append((float(d['total_loss'].detach()), float(gn)))
        d, gn = (step(img, mask) if graphed else train_iteration(model, opt, scaler, img, mask, double_step=True))
        log.append((float(d['total_loss'].detach()), float(gn)))
    return log, {k: v.detach().clone() for k, v in model.state_dict().items()}, ema, step


def test_captured_step_updates_the_shadows_like_the_eager_loop(hip):
    batches = _batches(6, 2, 96, 128)
    odd = (4, _batches(1, 3, 96, 128)[0])
    plain = _pspnet(torch.float32)
    eager, graph = copy.deepcopy(plain), copy.deepcopy(plain)
    log_p, sd_p, _, _ = _run(plain, batches, False, False, odd)
    log_e, sd_e, ema_e, _ = _run(eager, batches, False, True, odd)
    log_g, sd_g, ema_g, step = _run(graph, batches, True, True, odd)
    assert step.graph is not None and step.replays >= 4, 'the step was never replayed from a graph'
    assert ema_g._captured and ema_e.updates == ema_g.updates == 7
    tracked = [k for k, p in plain.named_parameters() if p.requires_grad] + [k for k in sd_p if k.endswith('running_mean') or k.endswith('running_var')]
    assert sorted(ema_g.names) == sorted(tracked) and len(tracked) > 250
    for k in ema_e.names:
        assert torch.equal(ema_e.shadows[k], ema_g.shadows[k]), k
    assert any(not torch.equal(ema_g.shadows[k], sd_g[k]) for k in ema_g.names)
    # the EMA changes nothing of the training itself
    assert log_p == log_e == log_g, (log_p, log_e, log_g)
    for k in sd_p:
        assert torch.equal(sd_p[k], sd_e[k]) and torch.equal(sd_p[k], sd_g[k]), k


def test_captured_ft_step_updates_the_shadows_like_the_eager_loop(hip):
    """ft_pop's loop body with the HIP SGD inside the graph and a learning rate that changes every iteration; the frozen backbone is not tracked"""
    from segland_amd import graph_step
    from segland_amd.ema import ModelEma
    from segland_amd.ft_pop import ft_graph_body, ft_iteration, ft_iteration_graphed
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.networks.pspnet_pop import GFSS_Model
    from segland_amd.optim import SGD
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    H, W = 96, 128
    plain = GFSS_Model(n_base=7, criterion=OrthLoss(255), pretrained_model=None, is_ft=True, n_novel=4, compute_dtype=torch.float32, backbone='resnet50', dilated=True, os=8)
    fm.load_formula_weights(plain)
    plain = plain.to(DEV)
    plain.init_cls_n()
    eager, graph = copy.deepcopy(plain), copy.deepcopy(plain)
    data = []
    for k in range(6):
        img = fm.formula_image(2, H, W, 'gf/img%d' % k).to(DEV)
        img_b = fm.formula_image(2, H, W, 'gf/imgb%d' % k).to(DEV)
        mask = (fm.formula_mask(2, H, W, 4, 'gf/mask%d' % k, block=16, ignore_rows=4) + 8)
        mask[mask > 11] = 255
        mask_b = fm.formula_mask(2, H, W, 8, 'gf/maskb%d' % k, block=16, ignore_rows=0)
        data.append((img, mask.to(DEV), img_b, mask_b.to(DEV)))

    def run(model, graphed, with_ema):
        model.train_mode()
        opt = SGD(get_parameters(model, lr=1e-2, freeze_backbone=True), lr=1e-2, momentum=0.9, weight_decay=5e-4)
        opt.zero_grad()
        ema = None
        if with_ema:
            ema = ModelEma(model, 0.9)
            opt.attach_ema(ema)
        sc = NativeScalerWithGradNormCount()
        g = graph_step.GraphedStep(ft_graph_body(model, optimizer=opt), model, opt, warmup=2) if graphed else None
        log = []
        for k, (img, mask, img_b, mask_b) in enumerate(data):
            for grp in opt.param_groups:
                grp['lr'] = 1e-2 * (1 - k / 10.0)
            batch = (img, mask, img_b, mask_b.clone())
            d, gn = ft_iteration_graphed(g, opt, batch, DEV) if graphed else ft_iteration(model, opt, sc, batch, DEV)
            log.append((float(d['total_loss'].detach()), float(gn)))
        return log, {k: v.detach().clone() for k, v in model.state_dict().items()}, ema, g

    log_p, sd_p, _, _ = run(plain, False, False)
    log_e, sd_e, ema_e, _ = run(eager, False, True)
    log_g, sd_g, ema_g, g = run(graph, True, True)
    assert g.graph is not None and g.replays >= 4
    assert ema_e.updates == ema_g.updates == 6 and ema_g._captured
    assert sorted(ema_g.names) == ['classifier_n.0.weight', 'classifier_n.2.weight', 'classifier_n.4.weight', 'novel_emb']
    for k in ema_e.names:
        assert torch.equal(ema_e.shadows[k], ema_g.shadows[k]), k
        assert not torch.equal(ema_g.shadows[k], sd_g[k]), k
    assert log_p == log_e == log_g, (log_p, log_e, log_g)
    for k in sd_p:
        assert torch.equal(sd_p[k], sd_e[k]) and torch.equal(sd_p[k], sd_g[k]), k


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_applied_swaps_the_averaged_weights_in_and_out(hip, dtype):
    """After a few replays: eval logits inside applied() equal those of a deep copy loaded from model_state_dict(); after exit they equal those before entry, bit for bit
    (prepared GEMM copies, BN eval coefficients and the eval feature graph follow the exchange in both directions)"""
    batches = _batches(5, 2, 96, 128)
    model = _pspnet(dtype)
    fresh = copy.deepcopy(model)
    _, _, ema, step = _run(model, batches, True, True)
    assert step.replays >= 3 and ema.updates == 5
    fresh.load_state_dict(ema.model_state_dict(), strict=True)
    img = batches[0][0]

    def logits(m):
        m.eval()
        with torch.no_grad():
            return m(img).float().clone()

    want = logits(fresh)
    before = logits(model)
    with ema.applied():
        inside = logits(model)
        again = logits(model)
    after = logits(model)
    print('max |averaged - raw| logits: %.3g' % float((inside - before).abs().max()))
    assert not torch.equal(inside, before), 'the averaged weights did not reach the kernels'
    assert torch.equal(inside, want) and torch.equal(again, want)
    assert torch.equal(after, before), 'stale averaged weights / statistics after applied(): max diff %g' % float((after - before).abs().max())


# --------------------------------------------------------------------------------------------- drivers
BASE_FLAGS = ['--model', 'pspnet_pop', '--backbone', 'resnet50', '--dataset', 'synthetic', '--batch-size', '4', '--input-size', '128,128', '--base-size', '128,128',
              '--learning-rate', '1e-4', '--print-frequency', '4', '--num-workers', '0', '--restore-from', '/nonexistent', '--allow-random-init']


def test_train_base_with_ema_and_resume(hip, tmp_path):
    from segland_amd import train_base
    from segland_amd.networks.pspnet_pop import GFSS_Model
    from segland_amd.utils.pyt_utils import load_model
    snap = str(tmp_path / 'snap')
    train_base.main(BASE_FLAGS + ['--num-epoch', '1', '--snapshot-dir', snap, '--ema-decay', '0.99'])
    raw = torch.load(os.path.join(snap, 'epoch_1.pth'), map_location='cpu')
    avg = torch.load(os.path.join(snap, 'epoch_1_ema.pth'), map_location='cpu')
    assert list(raw) == list(avg) and all(torch.isfinite(v.float()).all() for v in avg.values())
    differ = [k for k in raw if not torch.equal(raw[k], avg[k])]
    assert 'module.base_emb' in differ and 'module.backbone.bn1.running_mean' in differ and not any(k.endswith('num_batches_tracked') for k in differ)
    m = GFSS_Model(n_base=7, backbone='resnet50', pretrained_model=None, dilated=True, os=8)
    load_model(m, os.path.join(snap, 'epoch_1_ema.pth'), is_restore=True)
    assert torch.equal(m.base_emb.detach(), avg['module.base_emb']) and torch.equal(m.backbone.bn1.running_mean, avg['module.backbone.bn1.running_mean'])
    state = torch.load(os.path.join(snap, 'state_1.pth'), map_location='cpu')
    assert state['ema']['updates'] == 16 and state['ema']['decay'] == 0.99 and state['ema']['warmup'] is True          # 64 tiles / batch 4
    assert torch.equal(state['state_dict']['module.base_emb'], raw['module.base_emb'])
    assert torch.equal(state['ema']['shadows']['module.base_emb'], avg['module.base_emb'])
    # -c continues the count (and the average)
    train_base.main(BASE_FLAGS + ['--num-epoch', '2', '--snapshot-dir', snap, '--ema-decay', '0.99', '-c', os.path.join(snap, 'state_1.pth')])
    state2 = torch.load(os.path.join(snap, 'state_2.pth'), map_location='cpu')
    assert state2['epoch'] == 2 and state2['ema']['updates'] == 32
    assert glob.glob(os.path.join(snap, 'epoch_2_ema.pth'))
    assert not torch.equal(state2['ema']['shadows']['module.base_emb'], state['ema']['shadows']['module.base_emb'])


def test_ft_pop_with_ema(hip, tmp_path):
    from segland_amd import ft_pop
    from segland_amd.networks.pspnet_pop import GFSS_Model
    from segland_amd.utils.pyt_utils import load_model
    snap = str(tmp_path / 'snap_ft')
    ft_pop.main(['--model', 'pspnet_pop', '--backbone', 'resnet50', '--dataset', 'synthetic', '--batch-size', '1', '--input-size', '128,128',
                 '--base-size', '128,128', '--num-epoch', '1', '--learning-rate', '1e-3', '--print-frequency', '5', '--snapshot-dir', snap,
                 '--num-workers', '0', '--restore-from', '/nonexistent', '--allow-random-init', '--random-seed', '123', '--freeze-backbone', '--fix-bn', '--update-base',
                 '--ema-decay', '0.99'])
    raw = torch.load(os.path.join(snap, 'epoch_0_123.pth'), map_location='cpu')
    avg = torch.load(os.path.join(snap, 'epoch_0_123_ema.pth'), map_location='cpu')
    assert list(raw) == list(avg)
    differ = sorted(k for k in raw if not torch.equal(raw[k], avg[k]))
    assert differ == ['module.classifier_n.0.weight', 'module.classifier_n.2.weight', 'module.classifier_n.4.weight', 'module.novel_emb'], differ
    m = GFSS_Model(n_base=7, backbone='resnet50', pretrained_model=None, dilated=True, os=8, is_ft=True, n_novel=avg['module.novel_emb'].shape[0])
    load_model(m, os.path.join(snap, 'epoch_0_123_ema.pth'), is_restore=True)
    assert torch.equal(m.novel_emb.detach(), avg['module.novel_emb'])
