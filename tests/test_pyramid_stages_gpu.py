"""The pyramid stage chain both decoders share (functional.stages_fwd / stages_bwd behind PPMFn and PspSwinFn): every hook route against the default route at module
level, the frozen forward, and the saved record across two forwards.  Shapes: the smallest at which the four levels (1, 2, 3, 6) are real and the 1x1 level's BatchNorm
sees more than two samples (B = 4)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def rel_l2(got, ref):
    got, ref = got.detach().float().cpu().double(), ref.detach().float().cpu().double()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-30))


def _resnet_run(dtype=torch.bfloat16):
    from segland_amd.functional import flush_num_batches_tracked
    from segland_amd.networks.pspnet_pop import PSPModule
    torch.manual_seed(4)
    dec = PSPModule(256, out_features=128).to(DEV).train()
    x = torch.randn(4, 12, 12, 256, device=DEV).to(dtype).requires_grad_(True)
    y = dec(x)
    flush_num_batches_tracked()
    (y.float() * torch.linspace(-1, 1, y.numel(), device=DEV).view_as(y)).sum().backward()
    return dec, x, y


def _swin_apply(psp, x, drop=None):
    from segland_amd.functional import flush_num_batches_tracked
    from segland_amd.functional_swin import PspSwinFn, psp_params
    y = PspSwinFn.apply(x, psp, drop, *psp_params(psp))
    flush_num_batches_tracked()
    return y


def _swin_module():
    from segland_amd.networks.swin_pop import PSPModule
    torch.manual_seed(4)
    return PSPModule(768, 96).to(DEV).train()


def _swin_run(dtype):
    psp = _swin_module()
    x = torch.randn(4, 6, 6, 768, device=DEV).to(dtype).requires_grad_(True)
    y = _swin_apply(psp, x)
    (y.float() * torch.linspace(-1, 1, y.numel(), device=DEV).view_as(y)).sum().backward()
    return psp, x, y


def _outcome(run, *args):
    mod, x, y = run(*args)
    grads = {k: p.grad.clone() for k, p in mod.named_parameters()} | {'x': x.grad.float().clone()}
    stats = {k: b.clone() for k, b in mod.named_buffers() if k.endswith(('running_mean', 'running_var'))}
    assert len(stats) == 2 * 5 and all(g.abs().max() > 0 for g in grads.values())
    return y.detach().clone(), grads, stats


_default = {}


def _against_default(key, run, args, module, hooks):
    """Runs `run` with the hooks (names in `module`) False and compares with the default route, which is computed once per key."""
    if key not in _default:
        _default[key] = _outcome(run, *args)
    was = {h: getattr(module, h) for h in hooks}
    try:
        for h in hooks:
            assert was[h] is True, h
            setattr(module, h, False)
        y, grads, stats = _outcome(run, *args)
    finally:
        for h in hooks:
            setattr(module, h, was[h])
    y0, grads0, stats0 = _default[key]
    errs = {k: rel_l2(grads[k], grads0[k]) for k in grads0}
    worst = max(errs, key=errs.get)
    print('  %s, %s off: worst gradient %s relative L2 %.2e' % (key, ' + '.join(hooks), worst, errs[worst]))
    assert torch.equal(y, y0), 'the hooks touch the backward only'
    for k in stats0:
        assert torch.equal(stats[k], stats0[k]), k
    for k, e in errs.items():
        assert e <= 1e-4, (k, e)


@pytest.mark.parametrize('hooks', [('_STAGE_BN_GROUPED',), ('_PPM_WGRAD_GROUPED',), ('_STAGE_BN_GROUPED', '_PPM_WGRAD_GROUPED')], ids='+'.join)
def test_resnet_pyramid_hook_routes(hip, hooks):
    """pspnet_pop.PSPModule: the per-level BatchNorm backward and / or the per-level stage weight gradients against the grouped launches.  Every parameter gradient and the
    input gradient to 1e-4 relative L2 per tensor (the stage path is fp32, the routes differ in summation order only: the gate of test_ppm_rows_weight_gradients_grouped);
    output and running statistics bit-equal."""
    from segland_amd import functional as sf
    _against_default('resnet', _resnet_run, (), sf, hooks)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_swin_pyramid_hook_route(hip, dtype):
    """swin_pop.PSPModule (PspSwinFn): _PSP_GROUPED off, the per-level chain, against the two grouped launches; same gates."""
    from segland_amd import functional_swin as fs
    _against_default('swin %s' % dtype, _swin_run, (dtype,), fs, ('_PSP_GROUPED',))


def test_resnet_pyramid_frozen_forward(hip):
    """PPMFn's _frozen call (eval mode, no gradient wanted) goes through the shared forward and keeps nothing: the output is that of a second module in eval mode that
    received the same state through load_state_dict, bit for bit, and has no grad_fn."""
    from segland_amd.networks.pspnet_pop import PSPModule
    dec, x, _ = _resnet_run()                       # one train-mode step first: the running statistics are not the initial 0 / 1
    twin = PSPModule(256, out_features=128).to(DEV)
    twin.load_state_dict(dec.state_dict())
    dec.eval(), twin.eval()
    with torch.no_grad():
        y, y2 = dec(x.detach()), twin(x.detach())
    assert y.grad_fn is None and y2.grad_fn is None
    assert torch.isfinite(y.float()).all() and float(y.float().abs().max()) > 0
    assert torch.equal(y, y2)


def test_swin_pyramid_record_belongs_to_its_forward(hip):
    """Two forwards of one swin_pop.PSPModule before the first backward, then both backwards: gradients bit-equal to two independent single passes accumulated in the
    same order (what the forward keeps travels in its own ctx, not on the module)."""
    g = torch.Generator(device='cpu').manual_seed(6)
    xs = [torch.randn(4, 6, 6, 768, generator=g).to(DEV) for _ in range(2)]
    drop = (torch.rand(4, 96, generator=g) > 0.1).float().div(0.9).to(DEV)
    coef = torch.linspace(-1, 1, 4 * 6 * 6 * 128, device=DEV).view(4, 6, 6, 128)

    def grads(interleaved):
        psp = _swin_module()
        ins = [x.clone().requires_grad_(True) for x in xs]
        if interleaved:
            ys = [_swin_apply(psp, x, drop) for x in ins]
            for k, y in enumerate(ys):
                (y * coef * (k + 1)).sum().backward()
        else:
            for k, x in enumerate(ins):
                (_swin_apply(psp, x, drop) * coef * (k + 1)).sum().backward()
        return {k: p.grad for k, p in psp.named_parameters()} | {'x%d' % k: x.grad for k, x in enumerate(ins)}
    got, ref = grads(True), grads(False)
    for k in ref:
        assert float(ref[k].abs().max()) > 0, k
        assert torch.equal(got[k], ref[k]), (k, rel_l2(got[k], ref[k]))
