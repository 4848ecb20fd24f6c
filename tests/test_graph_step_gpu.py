"""The training step replayed as ONE HIP graph (segland_amd/graph_step.py) against the same step issued kernel by kernel: identical
losses, gradient norms, parameters, AdamW moments and step counts -- with a different batch every step (static-input copies), a learning
rate changed between replays (device-side hyper-parameters), an eager step of another shape in between, and evaluation afterwards (stale
weight copies).  PSPNet-POP in fp32 and bf16, Swin-POP with fixed DropPath / Dropout2d scales."""
import copy

import pytest
import torch

from oracle import formula as fm

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _pspnet(dtype):
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.networks.pspnet_pop import GFSS_Model
    m = GFSS_Model(n_base=7, criterion=OrthLoss(255), backbone='resnet50', pretrained_model=None, dilated=True, os=8, compute_dtype=dtype)
    fm.load_formula_weights(m)
    return m.to(DEV).train()


def _swin(dtype):
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.networks.swin_pop import GFSS_Model
    m = GFSS_Model(n_base=7, criterion=OrthLoss(255), backbone='swin-t', pretrained_model=None, compute_dtype=dtype)
    fm.load_formula_weights(m)
    m = m.to(DEV).train()
    # fixed stochastic-depth / Dropout2d scales: the graph's Philox draws differ from an eager run's, the comparison must not
    m.backbone.drop_path_hook = lambda index, B, p: torch.full((B,), 1.0, device=DEV)
    m.decoder.dropout2d_hook = lambda B, Cn, p: torch.full((B, Cn), 1.0, device=DEV)
    return m


def _batches(n, B, H, W):
    out = []
    for k in range(n):
        img = fm.formula_image(B, H, W, 'gs/img%d' % k).to(DEV)
        mask = fm.formula_mask(B, H, W, 8, 'gs/mask%d' % k, block=16, ignore_rows=4).to(DEV)
        out.append((img, mask))
    return out


def _run(model, batches, graphed, lr_change_at, odd=None):
    from segland_amd import graph_step
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    opt = AdamW(get_parameters(model, lr=1e-4), lr=1e-4, weight_decay=1e-4)
    scaler = NativeScalerWithGradNormCount()
    step = graph_step.GraphedTrainStep(train_iteration, model, opt, scaler, double_step=True, warmup=2) if graphed else None
    log = []
    for k, (img, mask) in enumerate(batches):
        if k == lr_change_at:
            for i, g in enumerate(opt.param_groups):
                g['lr'] = 3e-5 * (1 + i)
        if odd is not None and k == odd[0]:                      # a batch of another shape: runs eagerly, the graph survives it
            d, gn = (step(*odd[1]) if graphed else train_iteration(model, opt, scaler, *odd[1], double_step=True))
            log.append((float(d['total_loss'].detach()), float(gn)))
        d, gn = (step(img, mask) if graphed else train_iteration(model, opt, scaler, img, mask, double_step=True))
        log.append((float(d['total_loss'].detach()), float(gn)))
    model.eval()
    with torch.no_grad():
        logits = model(batches[0][0]).float().cpu()
    return log, {k: v.detach().float().cpu() for k, v in model.state_dict().items()}, opt, logits, step


@pytest.mark.parametrize('family,dtype', [('pspnet', torch.float32), ('pspnet', torch.bfloat16), ('swin', torch.float32), ('swin', torch.bfloat16)])
def test_graphed_step_equals_eager(hip, family, dtype):
    build = _pspnet if family == 'pspnet' else _swin
    H, W = (96, 128) if family == 'pspnet' else (128, 160)
    batches = _batches(6, 2, H, W)
    odd = (4, _batches(1, 3, H, W)[0])
    ref = build(dtype)
    got = copy.deepcopy(ref)
    if family == 'swin':
        got.backbone.drop_path_hook, got.decoder.dropout2d_hook = ref.backbone.drop_path_hook, ref.decoder.dropout2d_hook
    log_r, sd_r, opt_r, logits_r, _ = _run(ref, batches, False, 3, odd)
    log_g, sd_g, opt_g, logits_g, step = _run(got, batches, True, 3, odd)
    assert step.graph is not None and step.replays >= 4, 'the step was never replayed from a graph'
    print('losses / grad norms eager vs graph:', log_r, log_g)
    assert log_r == log_g                                         # same kernels in the same order on the same data: bit-identical
    for k in sd_r:
        assert torch.equal(sd_r[k], sd_g[k]), k
    assert torch.equal(logits_r, logits_g)
    for (pr, sr), (pg, sg) in zip(opt_r.state.items(), opt_g.state.items()):
        assert float(sr['step']) == float(sg['step']) and torch.equal(sr['exp_avg'], sg['exp_avg']) and torch.equal(sr['exp_avg_sq'], sg['exp_avg_sq'])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_validation_between_replays_sees_fresh_weights_and_statistics(hip, dtype):
    """train (replays) -> eval -> train (replays ONLY) -> eval: a replay runs no Python, so neither the optimizer post-step hook nor
    _bn_coeffs bump the host-side cache keys; the second evaluation must still use the weights, the prepared GEMM copies, the BN running
    statistics and a fresh eval feature graph of THAT moment (train_base validates every 10 epochs through exactly this sequence)."""
    from segland_amd import graph_step
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    batches = _batches(8, 2, 96, 128)

    def run(model, graphed):
        opt = AdamW(get_parameters(model, lr=1e-3), lr=1e-3, weight_decay=1e-4)
        sc = NativeScalerWithGradNormCount()
        step = graph_step.GraphedTrainStep(train_iteration, model, opt, sc, double_step=True, warmup=2) if graphed else None
        evals = []
        for phase in (batches[:5], batches[5:]):
            model.train()
            for img, mask in phase:
                step(img, mask) if graphed else train_iteration(model, opt, sc, img, mask, double_step=True)
            model.eval()
            with torch.no_grad():
                evals.append(model(batches[0][0]).float().cpu())
        return evals, step

    ref = _pspnet(dtype)
    got = copy.deepcopy(ref)
    ev_r, _ = run(ref, False)
    ev_g, step = run(got, True)
    assert step.replays >= 5 and step.graph is not None
    assert not torch.equal(ev_r[0], ev_r[1])                      # the second phase really moved the model
    assert torch.equal(ev_r[0], ev_g[0])
    assert torch.equal(ev_r[1], ev_g[1]), 'second validation used stale weights / running statistics: max diff %g' % float((ev_r[1] - ev_g[1]).abs().max())


def test_graphed_step_draws_fresh_stochastic_depth(hip):
    """DropPath / Dropout2d inside the graph draw new masks on every replay (torch's graph-safe Philox offsets): two replays on the SAME
    batch with the learning rate at 0 give different losses in train mode."""
    from segland_amd import graph_step
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    m = _swin(torch.float32)
    m.backbone.drop_path_hook = m.decoder.dropout2d_hook = None
    opt = AdamW(get_parameters(m, lr=0.0), lr=0.0, weight_decay=0.0)
    step = graph_step.GraphedTrainStep(train_iteration, m, opt, NativeScalerWithGradNormCount(), warmup=2)
    img, mask = _batches(1, 2, 128, 160)[0]
    losses = [float(step(img, mask)[0]['total_loss']) for _ in range(5)]
    print(losses)
    assert step.replays >= 3 and len(set(losses[2:])) > 1


@pytest.mark.parametrize('family,sgd', [('pspnet', 'hip'), ('swin', 'hip'), ('pspnet', 'torch')])
def test_graphed_ft_step_equals_eager(hip, family, sgd):
    """ft_pop loop body (ft_pop.py:243-256): forward_novel + forward_all on a (novel, base) pair with in-place pseudo-labels, backward,
    clip_grad_norm_ and the SGD step replayed from ONE graph with a learning rate that changes every iteration (segland_amd.optim.SGD reads it from device
    memory) -- against the kernel-by-kernel loop body: losses, gradient norms and parameters bit for bit.  (segland_amd.optim.SGD against torch.optim.SGD, the
    reference's optimizer: test_sgd_kernel_equals_torch_sgd.)  sgd='torch': torch's SGD behind the replay (round 3's arrangement, still what a caller-supplied torch
    optimizer gets)."""
    from segland_amd import graph_step
    from segland_amd.ft_pop import ft_graph_body, ft_iteration, ft_iteration_graphed
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    if family == 'pspnet':
        from segland_amd.networks.pspnet_pop import GFSS_Model
        kw, (H, W) = dict(backbone='resnet50', dilated=True, os=8), (96, 128)
    else:
        from segland_amd.networks.swin_pop import GFSS_Model
        kw, (H, W) = dict(backbone='swin-t'), (128, 160)
    ref = GFSS_Model(n_base=7, criterion=OrthLoss(255), pretrained_model=None, is_ft=True, n_novel=4, compute_dtype=torch.float32, **kw)
    fm.load_formula_weights(ref)
    ref = ref.to(DEV)
    ref.init_cls_n()
    got = copy.deepcopy(ref)
    data = []
    for k in range(6):
        img = fm.formula_image(2, H, W, 'gf/img%d' % k).to(DEV)
        img_b = fm.formula_image(2, H, W, 'gf/imgb%d' % k).to(DEV)
        mask = (fm.formula_mask(2, H, W, 4, 'gf/mask%d' % k, block=16, ignore_rows=4) + 8)
        mask[mask > 11] = 255
        mask_b = fm.formula_mask(2, H, W, 8, 'gf/maskb%d' % k, block=16, ignore_rows=0)
        data.append((img, mask.to(DEV), img_b, mask_b.to(DEV)))

    from segland_amd.optim import SGD

    def run(model, graphed):
        model.train_mode()
        ours = sgd == 'hip'                                  # the same optimizer on both sides: its eager launch and its captured launch are one kernel
        opt = (SGD if ours else torch.optim.SGD)(get_parameters(model, lr=1e-2, freeze_backbone=True), lr=1e-2, momentum=0.9, weight_decay=5e-4)
        opt.zero_grad()
        sc = NativeScalerWithGradNormCount()
        g = graph_step.GraphedStep(ft_graph_body(model, optimizer=opt if ours else None), model, opt if ours else None, warmup=2) if graphed else None
        log = []
        for k, (img, mask, img_b, mask_b) in enumerate(data):
            for grp in opt.param_groups:
                grp['lr'] = 1e-2 * (1 - k / 10.0)
            batch = (img, mask, img_b, mask_b.clone())
            d, gn = ft_iteration_graphed(g, opt, batch, DEV) if graphed else ft_iteration(model, opt, sc, batch, DEV)
            log.append((float(d['total_loss'].detach()), float(gn)))
        return log, {n: p.detach().float().cpu() for n, p in model.named_parameters() if p.requires_grad}, g

    log_r, par_r, _ = run(ref, False)
    log_g, par_g, g = run(got, True)
    print(log_r, log_g)
    assert g.graph is not None and g.replays >= 3
    assert log_r == log_g
    assert par_r.keys() == par_g.keys() and len(par_r) > 0
    for n in par_r:
        assert torch.equal(par_r[n], par_g[n]), n


def test_graphed_ft_step_behind_the_wrapper_recaptures_when_the_base_classifier_changes(hip):
    """What ft_pop.main really builds: GraphedStep and ft_graph_body on engine.ModuleWrapper(model) (engine.data_parallel on one GPU).  The frozen base classifier's
    prototype rows are cached tensors baked into the captured step (functional._base_chain); the lifecycle must look behind the wrapper for them: `baked` holds the cache
    entry the graph reads, and a change of classifier[0].weight in VALUE before iteration 4 (what load_state_dict / init_cls_n do behind a captured step) re-captures
    after two new warm-up steps instead of replaying the stale rows.  PSPNet-POP resnet50 fp32, os 8, pairs of 2 x 96 x 128, segland_amd.optim.SGD in the graph, ten
    iterations over six batches: losses, gradient norms and trainable parameters equal the kernel-by-kernel loop bit for bit."""
    from segland_amd import engine, graph_step
    from segland_amd.ft_pop import ft_graph_body, ft_iteration, ft_iteration_graphed
    from segland_amd.loss.criterion import OrthLoss
    from segland_amd.networks.pspnet_pop import GFSS_Model
    from segland_amd.optim import SGD
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    H, W = 96, 128
    ref = GFSS_Model(n_base=7, criterion=OrthLoss(255), pretrained_model=None, is_ft=True, n_novel=4, compute_dtype=torch.float32, backbone='resnet50', dilated=True, os=8)
    fm.load_formula_weights(ref)
    ref = ref.to(DEV)
    ref.init_cls_n()
    got = copy.deepcopy(ref)
    data = []
    for k in range(6):
        img = fm.formula_image(2, H, W, 'gf/img%d' % k).to(DEV)
        img_b = fm.formula_image(2, H, W, 'gf/imgb%d' % k).to(DEV)
        mask = (fm.formula_mask(2, H, W, 4, 'gf/mask%d' % k, block=16, ignore_rows=4) + 8)
        mask[mask > 11] = 255
        mask_b = fm.formula_mask(2, H, W, 8, 'gf/maskb%d' % k, block=16, ignore_rows=0)
        data.append((img, mask.to(DEV), img_b, mask_b.to(DEV)))

    def run(model, graphed):
        model.train_mode()
        opt = SGD(get_parameters(model, lr=1e-2, freeze_backbone=True), lr=1e-2, momentum=0.9, weight_decay=5e-4)
        opt.zero_grad()
        sc = NativeScalerWithGradNormCount()
        wrapped = engine.ModuleWrapper(model)
        g = graph_step.GraphedStep(ft_graph_body(wrapped, optimizer=opt), wrapped, opt, warmup=2) if graphed else None
        log = []
        for k in range(10):
            if k == 4:
                with torch.no_grad():
                    model.classifier[0].weight.mul_(1.5)
            for grp in opt.param_groups:
                grp['lr'] = 1e-2 * (1 - k / 10.0)
            img, mask, img_b, mask_b = data[k % 6]
            batch = (img, mask, img_b, mask_b.clone())
            d, gn = ft_iteration_graphed(g, opt, batch, DEV) if graphed else ft_iteration(model, opt, sc, batch, DEV)
            log.append((float(d['total_loss'].detach()), float(gn)))
            if graphed and k == 3:
                first.append((g.baked, g.replays))
        return log, {n: p.detach().float().cpu() for n, p in model.named_parameters() if p.requires_grad}, g

    first = []
    log_r, par_r, _ = run(ref, False)
    before = dict(graph_step.STATS)
    log_g, par_g, g = run(got, True)
    d = {k: graph_step.STATS[k] - before[k] for k in before}
    print(log_r, log_g, d)
    assert log_r == log_g, 'first differing iteration: %s' % [k for k in range(10) if log_r[k] != log_g[k]][:1]
    assert par_r.keys() == par_g.keys() and len(par_r) > 0
    for n in par_r:
        assert torch.equal(par_r[n], par_g[n]), n
    assert d == {'captures': 2, 'replays': 2 + 4, 'failures': 0}, d       # 0-1 warm-up, 2 capture, 3 replay, 4-5 warm-up again, 6 capture, 7-9 replays
    assert first[0][0] is not None and first[0][1] == 2, 'the first capture did not hold on to the base-chain cache entry'
    ent = got.__dict__.get('_sl_base_chain')
    assert g.baked is not None and g.baked is not first[0][0] and ent is not None and g.baked[0] == ent[0]
    assert len(ent[1]) == len(g.baked[1]) and all(a is b for a, b in zip(ent[1], g.baked[1])), 'the graph reads tensors that nothing keeps alive'


def test_train_base_replays_the_step_with_loader_workers(hip, tmp_path):
    """train_base.py end to end with the drivers' defaults that matter here -- DataLoader workers and the pin-memory thread alive while the
    step is captured (thread_local capture mode) -- must capture once and replay every later iteration; BatchNorm's num_batches_tracked,
    advanced inside the graph, counts all of them."""
    import glob
    import os
    from segland_amd import graph_step, train_base
    before = dict(graph_step.STATS)
    snap = str(tmp_path / 'snap')
    train_base.main(['--model', 'pspnet_pop', '--backbone', 'resnet50', '--dataset', 'synthetic', '--batch-size', '4', '--input-size', '128,128',
                     '--base-size', '128,128', '--num-epoch', '2', '--learning-rate', '1e-4', '--print-frequency', '4', '--snapshot-dir', snap,
                     '--num-workers', '2', '--restore-from', '/nonexistent', '--allow-random-init', '--fp16'])
    d = {k: graph_step.STATS[k] - before[k] for k in before}
    print(d)
    assert d['captures'] == 1 and d['failures'] == 0 and d['replays'] == 32 - 3, d          # 2 epochs x 16 iterations, 3 eager warm-up steps
    sd = torch.load(glob.glob(os.path.join(snap, 'epoch_2.pth'))[0], map_location='cpu')
    assert int(sd['module.backbone.bn1.num_batches_tracked']) == 32
    assert all(torch.isfinite(v.float()).all() for v in sd.values())


def test_failed_capture_falls_back_to_the_eager_step_and_recovers(hip):
    """A step whose body needs the host while it is being captured (a `.item()` read-back: hipErrorStreamCaptureUnsupported, the capture is invalidated) must run
    kernel by kernel as if nothing had happened -- graph_step clears the runtime's sticky error (csrc/api.cpp sl_hip_clear_error) so that the first launch check of
    the eager step does not report the capture's failure, and invalidates what the attempt left in host-side caches (functional.after_failed_capture: the attempt
    at iteration 3 fails AFTER the whole step was recorded) -- and the next attempt, with a well-behaved body, captures and replays.  Losses, gradient norms and
    parameters equal the plain eager run throughout."""
    from segland_amd import graph_step
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    batches = _batches(7, 2, 64, 96)
    ref = _pspnet(torch.float32)
    got = copy.deepcopy(ref)
    opt_r = AdamW(get_parameters(ref, lr=1e-4), lr=1e-4, weight_decay=1e-4)
    sc = NativeScalerWithGradNormCount()
    log_r = []
    for img, mask in batches:
        d, gn = train_iteration(ref, opt_r, sc, img, mask, double_step=True)
        log_r.append((float(d['total_loss'].detach()), float(gn)))
    opt_g = AdamW(get_parameters(got, lr=1e-4), lr=1e-4, weight_decay=1e-4)
    poison = ['early']

    def body(model, optimizer, scaler, img, mask, double_step=True):
        cap = torch.cuda.is_current_stream_capturing()
        if cap and poison[0] == 'early':
            img.sum().item()                                  # host read-back inside the capture, before anything of the step is recorded
        out = train_iteration(model, optimizer, scaler, img, mask, double_step=double_step)
        if cap and poison[0] == 'late':
            img.sum().item()                                  # ... and after ALL of it was recorded: weight copies, BN coefficients and counters of the attempt must not survive
        return out
    step = graph_step.GraphedTrainStep(body, got, opt_g, NativeScalerWithGradNormCount(), double_step=True, warmup=2)
    log_g = []
    for k, (img, mask) in enumerate(batches):
        if k == 3:
            poison[0] = 'late'
        if k == 4:
            poison[0] = None
        d, gn = step(img, mask)
        log_g.append((float(d['total_loss'].detach()), float(gn)))
        if k == 2:
            assert step.failures == 1 and step.graph is None, 'the poisoned capture did not fail'
    print(log_r, log_g, step.failures, step.replays)
    assert step.failures == 2 and step.graph is not None and step.replays >= 2          # attempts at iterations 2 and 3 fail, iteration 4 captures
    assert log_r == log_g
    for (k, a), (_, b) in zip(ref.state_dict().items(), got.state_dict().items()):
        assert torch.equal(a, b), k


def test_caller_touching_the_gradients_between_replays(hip):
    """VERDICT r4 (weak 11): GraphedStep re-points .grad at the captured tensors.  A caller of the drop-in may, between two replayed steps, (a) call
    optimizer.zero_grad(set_to_none=False) -- an in-place fill of the captured gradient tensors --, (b) clip or rescale the gradients OUTSIDE the graph
    (torch.nn.utils.clip_grad_norm_: in-place on the captured tensors, after the update the graph already applied), (c) drop them (zero_grad(): .grad = None).  None of it
    may change the following steps: every replay recomputes the gradients it uses.  Bit-identical to the kernel-by-kernel run."""
    from segland_amd import graph_step
    from segland_amd.optim import AdamW
    from segland_amd.train_base import train_iteration
    from segland_amd.utils.pyt_utils import NativeScalerWithGradNormCount, get_parameters
    batches = _batches(7, 2, 96, 128)
    ref = _pspnet(torch.float32)
    got = copy.deepcopy(ref)
    logs = {}
    for name, model, graphed in (('eager', ref, False), ('graph', got, True)):
        opt = AdamW(get_parameters(model, lr=1e-4), lr=1e-4, weight_decay=1e-4)
        scaler = NativeScalerWithGradNormCount()
        step = graph_step.GraphedTrainStep(train_iteration, model, opt, scaler, double_step=True, warmup=2) if graphed else None
        log = []
        for k, (img, mask) in enumerate(batches):
            d, gn = step(img, mask) if graphed else train_iteration(model, opt, scaler, img, mask, double_step=True)
            log.append((float(d['total_loss'].detach()), float(gn)))
            params = [p for p in model.parameters() if p.grad is not None]
            if k == 3:
                opt.zero_grad(set_to_none=False)
                assert all(float(p.grad.abs().max()) == 0.0 for p in params[:5])
            elif k == 4:
                torch.nn.utils.clip_grad_norm_(params, 0.01)
            elif k == 5:
                opt.zero_grad()
        if graphed:
            assert step.graph is not None and step.replays >= 4
        logs[name] = (log, {k: v.detach().float().cpu() for k, v in model.state_dict().items()})
    assert logs['eager'][0] == logs['graph'][0], (logs['eager'][0], logs['graph'][0])
    for k, v in logs['eager'][1].items():
        assert torch.equal(v, logs['graph'][1][k]), k
