"""Prepared weights of both model families: the one-launch refresh of a plan against the single-weight launch on fresh clones, the staleness rules (fused optimizers
and graph replays change weights without a version bump, frozen weights keep their copies, a re-pointed `.data` moves the storage), the few-stale routes.  Everything goes
through the names the models use: lin_prep, model_plan(...).refresh(), prepared, _PrepPlan.refresh, weights_changed.  Shapes: the smallest the batched kernel's 64 x 32
tiles allow, with every kind of entry (unpadded, padded 1x1 with bias, padded 3x3, column map)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _param(shape, seed, grad=True):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.nn.Parameter(torch.randn(shape, generator=g).to(DEV), requires_grad=grad)


def _swin_cases():
    """[(weight, bias, lin_prep keyword arguments)]: unpadded 1x1 128 -> 256 with bias; 1x1 96 -> 288 padded to 128 -> 320 with bias; 3x3 96 -> 96 padded to 128 -> 128;
    the decoder bottleneck's column map (two padded 96-channel maps and 128 channels: 320 real columns in 384)."""
    from segland_amd.functional_swin import _psp_colmap
    return [(_param((256, 128), 1), _param((256,), 2), {}),
            (_param((288, 96), 3), _param((288,), 4), {'Kp': 128, 'Np': 320}),
            (_param((96, 96, 3, 3), 5), None, {'Kp': 128, 'Np': 128, 'k': 3}),
            (_param((128, 320, 1, 1), 6), None, {'Kp': 384, 'col_map': _psp_colmap(96, 128, 2, 128, torch.device(DEV))})]


class _Registered:
    """lin_prep under a plan, as a model's forward runs it: refresh at the top, then the per-weight lookups."""

    def __init__(self, cases, dtype):
        from segland_amd import functional_swin as fs
        self.fs, self.cases, self.dtype = fs, cases, dtype
        self.plan = fs.model_plan(torch.nn.Module())
        self.forward(refresh=False)

    def forward(self, refresh=True):
        fs = self.fs
        if refresh:
            self.plan.refresh()
        fs.CURRENT_PLAN[0] = self.plan
        try:
            return [fs.lin_prep(w, b, self.dtype, **kw) for w, b, kw in self.cases]
        finally:
            fs.CURRENT_PLAN[0] = None

    def single(self, i):
        """The single-weight launch on fresh clones of case i's parameters, outside any plan."""
        w, b, kw = self.cases[i]
        clone = lambda p: None if p is None else torch.nn.Parameter(p.detach().clone())
        return self.fs.lin_prep(clone(w), clone(b), self.dtype, **kw)


def _same(L, R):
    return torch.equal(L.wf, R.wf) and torch.equal(L.wb, R.wb) and (L.bias is None) == (R.bias is None) and (L.bias is None or torch.equal(L.bias, R.bias))


def _count_batched(monkeypatch):
    from segland_amd import ops
    calls, real = [], ops.weight_prep_batched

    def counted(table, n, *a, **k):
        calls.append(n)
        return real(table, n, *a, **k)
    monkeypatch.setattr(ops, 'weight_prep_batched', counted)
    return calls


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_batched_refresh_equals_the_single_launch(hip, monkeypatch, dtype):
    reg = _Registered(_swin_cases(), dtype)
    calls = _count_batched(monkeypatch)
    with torch.no_grad():
        for w, b, _ in reg.cases:                       # an optimizer step in place
            w.mul_(0.5).add_(0.25)
            if b is not None:
                b.add_(1.0)
    reg.plan.refresh()
    assert calls == [4]                                  # all four stale: one launch for all
    Ls = reg.forward(refresh=False)
    assert calls == [4]
    for i, L in enumerate(Ls):
        assert _same(L, reg.single(i)), i
        w, b, kw = reg.cases[i]
        assert (L.N, L.K, L.Np, L.Kp, L.k) == (w.shape[0], w.shape[1], kw.get('Np', w.shape[0]), kw.get('Kp', w.shape[1]), kw.get('k', 1))
        assert tuple(L.wf.shape) == (L.Np, L.k, L.k, L.Kp) and tuple(L.wb.shape) == (L.Kp, L.k, L.k, L.Np) and L.wf.dtype == dtype
        real = torch.zeros(L.Kp, dtype=torch.bool, device=DEV)
        real[kw['col_map'] if 'col_map' in kw else slice(0, L.K)] = True
        assert float(L.wf[..., ~real].float().abs().sum()) == 0.0 and float(L.wb[~real].float().abs().sum()) == 0.0          # pad columns exactly zero
        assert float(L.wf[L.N:].float().abs().sum()) == 0.0 and float(L.wb[..., L.N:].float().abs().sum()) == 0.0            # pad rows exactly zero
        if b is not None:
            assert torch.equal(L.bias[:L.N], b.detach()) and float(L.bias[L.N:].abs().sum()) == 0.0
    # the real block is the parameter, rounded once
    L, (w, _, _) = Ls[3], reg.cases[3]
    assert torch.equal(L.wf[:, 0, 0][:, reg.cases[3][2]['col_map']], w.detach().view(128, 320).to(dtype))


def test_staleness_rules(hip):
    from segland_amd.functional import weights_changed
    dtype = torch.bfloat16
    # a write through .data bumps no version counter (a fused optimizer, a graph replay): weights_changed() makes the next refresh see it
    wt = _param((128, 128), 11)
    reg = _Registered([(wt, _param((128,), 13), {})], dtype)
    wt.data.mul_(-2.0)
    weights_changed()
    assert _same(reg.forward()[0], reg.single(0))
    # a frozen weight is not keyed on the epoch: same storage, same content -- also where the content behind it moved without a version bump
    wfz = _param((128, 128), 12, grad=False)
    reg = _Registered([(wfz, None, {})], dtype)
    Lf = reg.forward()[0]
    ptr, before = Lf.wf.data_ptr(), Lf.wf.clone()
    wfz.data.add_(1.0)
    weights_changed()
    Lf = reg.forward()[0]
    assert Lf.wf.data_ptr() == ptr and torch.equal(Lf.wf, before)
    # a version bump on it (load_state_dict: copy_ under no_grad) is picked up
    with torch.no_grad():
        wfz.copy_(wfz * 0.5)
    Lf = reg.forward()[0]
    assert _same(Lf, reg.single(0)) and not torch.equal(Lf.wf, before)
    # .data re-pointed to a new storage (a .to()): picked up, without any version bump or epoch
    wfz.data = wfz.data.clone().neg_()
    assert _same(reg.forward()[0], reg.single(0))


def test_few_stale_route_swin(hip, monkeypatch):
    """One stale weight of eight: the plan leaves it to lin_prep's own launch."""
    reg = _Registered([(_param((128, 128), 20 + i), _param((128,), 40 + i), {}) for i in range(8)], torch.bfloat16)
    calls = _count_batched(monkeypatch)
    ptrs = [L.wf.data_ptr() for L in reg.forward()]
    with torch.no_grad():
        reg.cases[5][0].mul_(3.0)
    Ls = reg.forward()
    assert calls == []
    assert _same(Ls[5], reg.single(5)) and [L.wf.data_ptr() for L in Ls] == ptrs


def _convs(shapes):
    return [torch.nn.Conv2d(i, o, k, bias=False).to(DEV) for i, o, k in shapes]


def test_few_stale_route_resnet(hip, monkeypatch):
    """One stale conv of eight after the first batched launch: a per-conv launch, the other seven keep their copies."""
    from segland_amd import functional as sf, ops
    torch.manual_seed(7)
    convs, dts = _convs([(64, 64, 1)] * 8), [torch.bfloat16] * 8
    calls = _count_batched(monkeypatch)
    plan = sf._PrepPlan()
    plan.refresh(convs, dts)
    ptrs = [sf.prepared(c.weight, d)[0].data_ptr() for c, d in zip(convs, dts)]
    with torch.no_grad():
        convs[2].weight.add_(1.0)
    plan.refresh(convs, dts)
    assert calls == [8]
    wf, wb = sf.prepared(convs[2].weight, torch.bfloat16)
    rf, rb = ops.weight_prep(convs[2].weight.detach().clone(), torch.bfloat16)
    assert torch.equal(wf, rf) and torch.equal(wb, rb)
    assert [sf.prepared(c.weight, d)[0].data_ptr() for k, (c, d) in enumerate(zip(convs, dts)) if k != 2] == ptrs[:2] + ptrs[3:]


def test_resnet_plan_follows_a_changed_weight_in_the_same_buffers(hip):
    from segland_amd import functional as sf, ops
    torch.manual_seed(8)
    convs, dts = _convs([(64, 128, 3), (96, 64, 1)]), [torch.bfloat16, torch.float32]
    plan = sf._PrepPlan()
    plan.refresh(convs, dts)
    first = [sf.prepared(c.weight, d) for c, d in zip(convs, dts)]
    ptrs = [(wf.data_ptr(), wb.data_ptr()) for wf, wb in first]
    old = first[0][0].clone()
    convs[0].weight.data.mul_(-0.5)                     # no version bump
    sf.weights_changed()
    plan.refresh(convs, dts)
    for c, d, p in zip(convs, dts, ptrs):
        wf, wb = sf.prepared(c.weight, d)
        rf, rb = ops.weight_prep(c.weight.detach().clone(), d)
        assert torch.equal(wf, rf) and torch.equal(wb, rb)
        assert (wf.data_ptr(), wb.data_ptr()) == p      # an unchanged plan key: the same buffers, rewritten in place
    assert not torch.equal(sf.prepared(convs[0].weight, dts[0])[0], old)
