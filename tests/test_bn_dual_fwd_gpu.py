"""bn3 and the downsample BatchNorm of a stage's first bottleneck applied in one forward pass (csrc/bn.hip bn_act2_fwd_kernel, ops.bn_act2,
functional._BN_DUAL_FWD): bit-identical to the two ops.bn_act passes it replaces, at kernel level and through a whole block's forward and backward, and taken exactly
where both BatchNorms run on per-GPU batch statistics."""
import inspect

import pytest
import torch
import torch.nn as nn

from oracle import formula as fm

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# rows, C, dtype: FIXEDC with a tail chunk that is not full (32 000 vectors = 31.25 chunks of 1024); 12 channel vectors, 256 % 12 != 0: the per-vector coefficient
# path; fp32 (4 elements per vector); less than one chunk
KERNEL_SHAPES = [(1000, 256, torch.bfloat16), (77, 96, torch.bfloat16), (300, 64, torch.float32), (3, 64, torch.bfloat16)]
_two_pass = {}


def _operands(rows, C, dtype):
    g = torch.Generator(device='cpu').manual_seed(rows * 4099 + C)
    x, x2 = (torch.randn(rows, C, generator=g).to(DEV).to(dtype) for _ in range(2))
    # coefficients of both signs and of the operands' own scale: about half of the sums are negative (the ReLU and its bits matter) and the shortcut value has
    # bits below the bf16 mantissa (its rounding matters)
    sc, sh, sc2, sh2 = (torch.randn(C, generator=g).to(DEV) for _ in range(4))
    return x, sc, sh, x2, sc2, sh2


def _reference(rows, C, dtype, relu):
    """What the forward did before: the shortcut normalised into a tensor of its own, then bn3's pass with it as the residual.  Computed once per case."""
    from segland_amd import ops
    key = (rows, C, dtype, relu)
    if key not in _two_pass:
        x, sc, sh, x2, sc2, sh2 = _operands(rows, C, dtype)
        res = ops.bn_act(x2, sc2, sh2, relu=False)
        _two_pass[key] = ops.bn_act(x, sc, sh, residual=res, relu=relu, want_mask=True)
    return _two_pass[key]


@pytest.mark.parametrize('want_mask', [True, False])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('rows,C,dtype', KERNEL_SHAPES)
def test_bn_act2_equals_the_two_passes(hip, rows, C, dtype, relu, want_mask):
    from segland_amd import ops
    y_ref, mask_ref = _reference(rows, C, dtype, relu)
    r = ops.bn_act2(*_operands(rows, C, dtype), relu=relu, want_mask=want_mask)
    y, mask = r if want_mask else (r, None)
    assert y.dtype == dtype and torch.equal(y, y_ref)
    if relu:
        assert bool((y_ref == 0).any()) and bool((y_ref > 0).any())          # the ReLU cut something and passed something
    if want_mask and relu:
        assert mask.dtype == torch.uint8 and mask.numel() == rows * C * y.element_size() // 16 and torch.equal(mask, mask_ref)
    else:
        assert mask is None and (mask_ref is None) == (not relu)


# inplanes, planes, stride, dilation of tests/golden/g5_bottleneck_<name> (input 2 x inplanes x 16 x 16)
BLOCKS = {'s1_ds': (64, 64, 1, 1), 's2_ds': (256, 128, 2, 1), 'd2_ds': (512, 256, 1, 2)}


def _block(name, norm_layer=nn.BatchNorm2d):
    from segland_amd.networks.backbones.resnet import Bottleneck
    inp, pl, st, dil = BLOCKS[name]
    dsm = nn.Sequential(nn.Conv2d(inp, pl * 4, 1, stride=st, bias=False), norm_layer(pl * 4))
    blk = Bottleneck(inp, pl, stride=st, dilation=dil, downsample=dsm, norm_layer=norm_layer)
    blk.load_state_dict({k: fm.formula_tensor('g5' + name + '/' + k, v) for k, v in blk.state_dict().items()})
    return blk.to(DEV)


def _input(name, dtype):
    inp, pl, st, _ = BLOCKS[name]
    x = fm.sym('g5%s/x' % name, (2, inp, 16, 16), 1.0).relu_().permute(0, 2, 3, 1).contiguous().to(DEV).to(dtype)
    coef = fm.sym('g5%s/coef' % name, (2, pl * 4, 16 // st, 16 // st), 1.0).permute(0, 2, 3, 1).contiguous().to(DEV)
    return x, coef


class _Calls:
    """Counts ops.bn_act2 calls and the ops.bn_act calls of a downsample branch's own pass (the one bn_act call of a bottleneck without ReLU and without residual)."""

    def __init__(self, monkeypatch):
        from segland_amd import ops
        self.dual = self.shortcut = self.single = 0
        real_act, real_act2 = ops.bn_act, ops.bn_act2
        sig = inspect.signature(real_act)

        def bn_act(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            self.single += 1
            self.shortcut += (not b.arguments['relu']) and b.arguments['residual'] is None
            return real_act(*a, **k)

        def bn_act2(*a, **k):
            self.dual += 1
            return real_act2(*a, **k)
        monkeypatch.setattr(ops, 'bn_act', bn_act)
        monkeypatch.setattr(ops, 'bn_act2', bn_act2)

    def take(self):
        r = (self.dual, self.shortcut, self.single)
        self.dual = self.shortcut = self.single = 0
        return r


def _step(blk, x, coef):
    """One forward + backward -> every tensor the step produced."""
    from segland_amd.functional import flush_num_batches_tracked
    xg = x.clone().requires_grad_(True)
    y = blk(xg)
    (y.float() * coef).sum().backward()
    flush_num_batches_tracked()
    out = {'y': y.detach(), 'dx': xg.grad}
    out.update({'grad/' + k: p.grad for k, p in blk.named_parameters()})
    out.update({'buffer/' + k: b for k, b in blk.named_buffers()})
    return out


@pytest.mark.parametrize('name,dtype', [('s1_ds', torch.bfloat16), ('s2_ds', torch.bfloat16), ('d2_ds', torch.bfloat16), ('s2_ds', torch.float32)])
def test_stage_entry_block_is_bit_identical_with_the_dual_pass(hip, monkeypatch, name, dtype):
    from segland_amd import functional as sf
    calls = _Calls(monkeypatch)
    x, coef = _input(name, dtype)
    runs = {}
    for flag in (False, True):
        monkeypatch.setattr(sf, '_BN_DUAL_FWD', flag)
        runs[flag] = _step(_block(name).train(), x, coef)
        # on: one dual pass, no pass of the downsample branch's own, bn1 and bn2 as before; off: the four passes of the chain
        assert calls.take() == ((1, 0, 2) if flag else (0, 1, 4)), flag
    off, on = runs[False], runs[True]
    assert off.keys() == on.keys() and {'grad/bn3.weight', 'grad/downsample.0.weight', 'grad/downsample.1.bias', 'buffer/bn3.running_var',
                                        'buffer/downsample.1.running_mean', 'buffer/downsample.1.running_var'} <= on.keys()
    for k, v in off.items():
        assert v is not None and v.dtype == on[k].dtype and torch.equal(v, on[k]), k
    assert int(on['buffer/downsample.1.num_batches_tracked']) == 1 and float(on['y'].float().abs().sum()) > 0


def test_dual_pass_is_taken_only_on_per_gpu_batch_statistics(hip, monkeypatch):
    """Hook on throughout.  BatchNorms on their running statistics with a gradient still wanted: the chain of four ops.bn_act; a frozen block: the conv kernels apply
    the BatchNorms themselves; SyncBatchNorm semantics (a process group of two, stood in for as in test_model_gpu.py): the chain, whose statistics are all-reduced."""
    import torch.distributed as dist
    from segland_amd import functional as sf
    assert sf._BN_DUAL_FWD is True
    calls = _Calls(monkeypatch)
    x, coef = _input('s2_ds', torch.bfloat16)
    _step(_block('s2_ds').train(), x, coef)
    assert calls.take() == (1, 0, 2)
    _step(_block('s2_ds').eval(), x, coef)
    assert calls.take() == (0, 1, 4)
    blk = _block('s2_ds').eval().requires_grad_(False)
    with torch.no_grad():
        blk(x)
    assert calls.take() == (0, 0, 0)
    # SyncBatchNorm modules synchronise only when asked to (SEGLAND_SYNC_BN): without it they are per-GPU BatchNorms and take the dual pass
    _step(_block('s2_ds', nn.SyncBatchNorm).train(), x, coef)
    assert calls.take() == (1, 0, 2)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a, **k: 2)
    monkeypatch.setattr(dist, 'all_reduce', lambda t, *a, **k: t.mul_(2))
    sf.set_sync_bn('1')
    try:
        _step(_block('s2_ds', nn.SyncBatchNorm).train(), x, coef)
    finally:
        sf.set_sync_bn('0')
    assert calls.take() == (0, 1, 4)
