"""Block-level autograd Functions: each one runs a fused chain of libsegland_hip.so kernels forward and the
hand-written backward chain, so PyTorch's autograd only links blocks together and accumulates parameter gradients
(which is what lets DDP's bucketed RCCL all-reduce overlap with the backward of earlier blocks).

nn.Conv2d / nn.BatchNorm2d modules are used purely as parameter holders (state_dict compatibility with the
reference); their own forward is never called.
"""
import os
from collections import namedtuple

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .ops import ConvSpec

_nbt_pending = []       # num_batches_tracked buffers to bump once per forward

# Staleness of the derived (GEMM-layout / compute-dtype) weight copies.  The tensor version counter alone is not enough: fused
# optimizers (torch.optim.AdamW(fused=True), the drivers' default on the GPU) update parameters WITHOUT bumping `_version`.  A global
# post-step hook on every torch optimizer advances an epoch that is part of the cache key of trainable weights; frozen weights
# (requires_grad False: the ft_pop backbone) keep their copies across steps, load_state_dict still bumps their version.
_OPT_EPOCH = [0]


def _on_optimizer_step(optimizer, args, kwargs):
    _OPT_EPOCH[0] += 1


from torch.optim.optimizer import register_optimizer_step_post_hook as _register_post_step      # noqa: E402

_register_post_step(_on_optimizer_step)


def weights_changed():
    """For code that mutates parameters behind torch's back (`.data` writes, custom optimizers that are not torch.optim subclasses,
    HIP-graph replays that contain an optimizer step: no Python hook runs during a replay)."""
    _OPT_EPOCH[0] += 1


# BatchNorm running statistics are written by kernels through raw pointers.  An eager train-mode forward bumps the module's own
# `_sl_rs_epoch`; a HIP-graph replay runs no Python at all, so graph_step bumps this global epoch after every replay.  It is part of
# the key of every cache derived from running statistics (_bn_eval_coeffs, GFSS_Model._features_graphed).
_RS_EPOCH = [0]


def running_stats_changed():
    _RS_EPOCH[0] += 1


def _wver(w):
    if w is None:
        return None
    return (w._version, _OPT_EPOCH[0] if w.requires_grad else 0)


def prepared(w, dtype):
    """GEMM-layout copies of a conv weight in the compute dtype, refreshed when the parameter changes.
    The cache lives on the Parameter object itself (version counter + storage pointer + dtype as the key)."""
    ent = getattr(w, '_sl_prep', None)
    if ent is None or ent[0] != _wver(w) or ent[1] != dtype or ent[2] != w.data_ptr():
        wf, wb = ops.weight_prep(w, dtype)
        ent = (_wver(w), dtype, w.data_ptr(), wf, wb)
        w._sl_prep = ent
    return ent[3], ent[4]


class _PrepPlan:
    """All conv weights of a model -> GEMM layouts in one kernel launch per optimizer step (instead of one per conv)."""

    def __init__(self):
        self.key, self.table, self.total, self.items = None, None, 0, []

    def refresh(self, convs, dtypes):
        import struct
        ws = [c.weight for c in convs]
        stale = [(w, d) for w, d in zip(ws, dtypes) if (getattr(w, '_sl_prep', None) is None or w._sl_prep[0] != _wver(w)
                                                         or w._sl_prep[1] != d or w._sl_prep[2] != w.data_ptr())]
        if not stale:
            return
        if len(stale) * 4 < len(ws) and self.key is not None:   # a few trainable weights over a frozen backbone (ft_pop): per-conv launches
            for w, d in stale:
                prepared(w, d)
            return
        key = tuple((w.data_ptr(), d) for w, d in zip(ws, dtypes))
        if key != self.key:                                   # (re)build buffers + the device table
            rec, start, self.items = b'', 0, []
            for w, d in zip(ws, dtypes):
                O, I, KH, KW = w.shape
                wf = torch.empty((O, KH, KW, I), dtype=d, device=w.device)
                wb = torch.empty((I, KH, KW, O), dtype=d, device=w.device)
                rec += struct.pack('<QQQiiiiq', w.data_ptr(), wf.data_ptr(), wb.data_ptr(), O, I, KH * KW, ops.dt(d), start)
                assert O % 64 == 0 and I % 32 == 0 and KH * KW <= 9
                start += O * I // 2048
                self.items.append((w, d, wf, wb))
            self.table = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(ws[0].device)
            self.total, self.key = start, key
        ops.weight_prep_batched(self.table, len(self.items), self.total,
                                nbytes=sum(w.numel() * (4 + 2 * wf.element_size()) for w, _, wf, _ in self.items))
        for w, d, wf, wb in self.items:
            w._sl_prep = (_wver(w), d, w.data_ptr(), wf, wb)


def refresh_weights(model):
    """Called once per forward by GFSS_Model: re-derives the GEMM-layout copies of every conv weight whose version changed."""
    plan = model.__dict__.get('_sl_prep_plan')
    if plan is None:
        plan = model.__dict__['_sl_prep_plan'] = _PrepPlan()
        convs, dtypes = [], []
        stage_convs = {id(st[1]) for st in model.decoder.stages}
        for m in list(model.backbone.modules()) + list(model.decoder.modules()) + list(model.classifier.modules()) + \
                (list(model.classifier_n.modules()) if getattr(model, 'classifier_n', None) is not None else []):
            if isinstance(m, torch.nn.Conv2d) and m.kernel_size[0] in (1, 3) and m.out_channels % 64 == 0 and m.in_channels % 32 == 0 \
                    and not (_PPM_FACTORISED and m is model.decoder.bottleneck[0]):       # that one is consumed as slices (_ppm_weights)
                convs.append(m)
                dtypes.append(torch.float32 if id(m) in stage_convs else model.compute_dtype)     # PPM stage path is fp32
        plan.convs, plan.dtypes = convs, dtypes
    if all(w.weight.is_cuda and w.weight.dtype == torch.float32 and w.weight.is_contiguous() for w in plan.convs):
        plan.refresh(plan.convs, plan.dtypes)


# ---- gradients written in place into DDP's bucket views --------------------------------------------------------------------------------
# Under DistributedDataParallel(gradient_as_bucket_view=True) a parameter's .grad is a view into the flat bucket the RCCL all-reduce runs on.
# The engine caches those views on the parameters (`_sl_gview`, refreshed before every optimizer step); a block backward that finds one
# lets its kernels write the gradient THERE and hands autograd a fresh alias of it: AccumulateGrad adopts the alias without a copy and
# DDP's reducer, seeing `grad.is_alias_of(bucket_view)`, neither copies nor (with the engine's sum-only comm hook) scales it -- the ~290
# per-parameter copy / scale kernels of a plain DDP step disappear.  Correct whatever the cache holds: DDP compares storages itself and
# falls back to its copy when the view is stale (the one iteration after it rebuilt its buckets).
def grad_dst(p):
    v = getattr(p, '_sl_gview', None)
    if v is None or v.shape != p.shape or v.dtype != torch.float32 or not v.is_contiguous() or p.grad is not None:
        return None                                    # p.grad set already (gradient accumulation): autograd must ADD, so no in-place write
    return v


def grad_alias(t, dst):
    """What a backward returns for a gradient it wrote into `dst` (a cached bucket view): a new tensor object on the same storage."""
    return t.detach() if (dst is not None and t is dst) else t


def flush_num_batches_tracked():
    """One launch for the counters of every train-mode BatchNorm that ran since the last flush (the models call it at the end of their feature extractor).
    The step drivers also call it right BEFORE they start a graph capture: an entry left behind by code that ran BatchNorm layers outside a model's forward (unit
    tests of single blocks) would otherwise be bumped by a node of the new graph -- on every replay, for as long as the graph lives, whatever has become of the
    module that owned the counter."""
    if _nbt_pending:
        torch._foreach_add_(_nbt_pending, 1)
        _nbt_pending.clear()


def discard_pending_counters():
    """After a FAILED graph capture: the BatchNorm layers of the attempt queued their counters, but nothing of the attempt ran (the step is about to be issued again,
    kernel by kernel, and queues them again)."""
    _nbt_pending.clear()


def after_failed_capture():
    """Host-side state a failed capture attempt leaves behind: queued BatchNorm counters (nothing of the attempt ran) and cache entries whose CONTENT was to be produced
    by captured launches -- prepared weight copies, BN evaluation coefficients -- under keys that would still match in the eager step that follows."""
    discard_pending_counters()
    weights_changed()
    running_stats_changed()


def spec_of(conv):
    return ConvSpec(conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0])


def _bn_coeffs(bn, part, count):
    """(mean, invstd, scale, shift) for this call; train mode also updates the running statistics."""
    if bn.training:
        world = sync_world(bn)
        # torch checks the GLOBAL count under SyncBatchNorm (nn/modules/_functions.py) and the local one under BatchNorm2d
        # (F.batch_norm): with SEGLAND_SYNC_BN=1 a per-GPU batch of 1 (PPM level 1: B*1*1 values per channel) trains, without it raises
        if count * max(world, 1) <= 1:
            raise ValueError('Expected more than 1 value per channel when training, got %d (per-GPU batch 1 needs SEGLAND_SYNC_BN=1: '
                             'the default BatchNorm statistics are per GPU)' % count)
        if bn.momentum is None:
            raise RuntimeError('segland_amd: cumulative-average BatchNorm (momentum=None) is not supported')
        if world:                                            # SyncBatchNorm: global sum / sum of squares / count (equal shards)
            part, count = ops.allreduce_partials(part), count * world
        out = ops.bn_finalize_train(part, count, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)
        _nbt_pending.append(bn.num_batches_tracked)
        # the kernel wrote the running statistics through raw pointers (no tensor version bump): invalidate the eval-coefficient cache
        bn.__dict__['_sl_rs_epoch'] = bn.__dict__.get('_sl_rs_epoch', 0) + 1
        return out
    return _bn_eval_coeffs(bn)


_SYNC_BN = os.environ.get('SEGLAND_SYNC_BN', '0')


def set_sync_bn(mode):
    """'0' (per-GPU statistics, default), '1' (synchronise nn.SyncBatchNorm modules when world_size > 1) or 'force' (also at world_size 1)."""
    global _SYNC_BN
    _SYNC_BN = str(mode)


def sync_world(bn):
    """World size if this BN synchronises its batch statistics over the process group, else 0.  Default: statistics are per GPU
    (DESIGN.md section 6); SEGLAND_SYNC_BN=1 gives nn.SyncBatchNorm modules the reference's distributed semantics (train_base.py:175-176)
    at the price of two small all-reduces per layer and direction."""
    if _SYNC_BN == '0' or not bn.training or not isinstance(bn, torch.nn.SyncBatchNorm):
        return 0
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    w = dist.get_world_size()
    return w if (w > 1 or _SYNC_BN == 'force') else 0


# What the forward of one BatchNorm(+ReLU) layer keeps for its backward: the conv output c the BatchNorm read, its batch (or running) mean / invstd and the ReLU bits
# of its output (None: no ReLU, or the mask was not asked for).
BNLayer = namedtuple('BNLayer', 'c mean invstd bits')


class Grad:
    """A gradient on its way down the backward chain: the tensor t, its ReLU gate still to be applied -- `bits` (the bit mask of the forward) or `act` (the activation
    itself: y > 0) or neither (no ReLU, or gated already) -- and the BatchNorm-backward column sums that came with it from the epilogue that wrote it (part; part2: those
    of a second BatchNorm behind the same ReLU).  A gradient that arrives with column sums is already gated."""
    __slots__ = ('t', 'bits', 'act', 'part', 'part2')

    def __init__(self, t, part=None, part2=None, bits=None, act=None):
        assert (part is None or (bits is None and act is None)) and (bits is None or act is None) and (part2 is None or part is not None)
        self.t, self.bits, self.act, self.part, self.part2 = t, bits, act, part, part2


# What the forward of a pyramid's stages (stages_fwd) keeps for stages_bwd: the pooled rows, the stage convs' output `call` and the activations stage_act (fp32
# [rows][pitch], the levels' rows one after the other) and per level the BatchNorm's mean / invstd.
StageRec = namedtuple('StageRec', 'pooled call stage_act mean invstd')


def _save(ctx, *items):
    """ctx.save_for_backward of tensors, None, BNLayer / StageRec records and lists of tensors; _saved(ctx) gives the same sequence back."""
    groups = [[*it[:3], *it.mean, *it.invstd] if isinstance(it, StageRec) else it if isinstance(it, (list, BNLayer)) else [it] for it in items]
    ctx.saved_form = [(type(it), len(g)) for it, g in zip(items, groups)]
    ctx.save_for_backward(*[t for g in groups for t in g])


def _saved(ctx):
    sv = iter(ctx.saved_tensors)
    groups = [(kind, [next(sv) for _ in range(n)]) for kind, n in ctx.saved_form]
    return [BNLayer(*ts) if kind is BNLayer else StageRec(*ts[:3], ts[3:(len(ts) + 3) // 2], ts[(len(ts) + 3) // 2:]) if kind is StageRec
            else ts if kind is list else ts[0] for kind, ts in groups]


def conv_bn_fwd(x, conv, bn, relu, residual=None, x2=None, out=None, want_mask=False):
    """y = act(bn(conv(x)) (+ residual)) -> (y, BNLayer); want_mask: the record carries the ReLU bits."""
    wf, _ = prepared(conv.weight, x.dtype)
    c, part = ops.conv2d_fwd(x, wf, spec_of(conv), x2=x2, want_stats=bn.training)
    mean, invstd, scale, shift = _bn_coeffs(bn, part, c.numel() // c.shape[-1])
    r = ops.bn_act(c, scale, shift, residual=residual, relu=relu, out=out, want_mask=want_mask)
    y, mask = r if want_mask else (r, None)
    return y, BNLayer(c, mean, invstd, mask)


def conv_bn_infer(x, conv, bn, relu, residual=None, x2=None, out=None):
    """Frozen-statistics conv+BN(+residual)(+ReLU) as ONE kernel (no conv-output round trip, nothing saved)."""
    wf, _ = prepared(conv.weight, x.dtype)
    _, _, scale, shift = _bn_eval_coeffs(bn)
    return ops.conv2d_affine_fwd(x, wf, spec_of(conv), scale, shift, x2=x2, residual=residual, relu=relu, out=out)


def _bn_eval_coeffs(bn):
    """(mean, invstd, scale, shift) of a BN on its running statistics, cached on the module until any of its four tensors changes
    (58 tiny launches per frozen forward otherwise -- the ft_pop step is launch-bound)."""
    key = (_wver(bn.weight), _wver(bn.bias), bn.running_mean._version, bn.running_var._version, bn.running_mean.data_ptr(), bn.eps,
           bn.__dict__.get('_sl_rs_epoch', 0), _RS_EPOCH[0])      # train-mode forwards / graph replays update the statistics behind the version counters
    ent = bn.__dict__.get('_sl_eval')
    if ent is None or ent[0] != key:
        ent = (key, ops.bn_finalize_eval(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps))
        bn.__dict__['_sl_eval'] = ent
    return ent[1]


def _frozen(ctx, *bns):
    """True when nothing in this block needs a gradient and every BN runs on its running statistics."""
    return not any(ctx.needs_input_grad) and not any(b.training for b in bns)


_PPM_WGRAD_GROUPED = True  # test hook: the pyramid's eight row-GEMM weight gradients as two grouped launches (ops.ppm_rows_wgrad); False: one generic weight-gradient launch + slab reduce per level
_STAGE_BN_GROUPED = True   # test hook: the pyramid stages' BatchNorm backward in one launch (ops.ppm_stage_bn_bwd); SyncBatchNorm stages always take the per-level chain
_DS_HALF = True            # test hook: the data gradient of a stride-2 1x1 downsample conv stays on its own grid (conv2d_bwd_data_addend_half)
_BASE_CHAIN_CACHE = True   # test hook: ft mode, the frozen base classifier's rows are computed once (False: every iteration)
# The ONE environment switch of the BatchNorm-backward fusions (A/B of the whole feature against stand-alone reduce passes): SEGLAND_BN_FUSE=0 switches all three off.
# (The deep stem's pool backward is exempt: its kernel exists in the statistics-emitting form only, DeepStemFn.backward always takes bn3's column sums from it.)
_BN_FUSE = os.environ.get('SEGLAND_BN_FUSE', '1') != '0'        # BN-backward statistics in the data-gradient epilogues (conv_gemm_common.h: conv_epilogue_fast MODE 3)
_BN_DUAL = _BN_FUSE        # test hook: bn3 + downsample BN backward in one sweep each (bn.hip reduce2 / apply2)
_BN_DUAL_FWD = True        # test hook: bn3 + downsample BN forward apply in one pass (bn.hip bn_act2_fwd_kernel); False: the downsample branch's own pass writes the shortcut
_BN_CROSS = _BN_FUSE       # test hook: bn3's column sums from the NEXT block's conv1 data-gradient epilogue (pixel-stationary kernel MODE 5)
_PPM_FACTORISED = os.environ.get('SEGLAND_PPM_DIRECT') != '1'   # set_ppm_factorised: the prior half of the pyramid's 3x3 bottleneck conv contracted on the s x s grids


def _bn_bwd(g, layer, bn, need_w, want_dres=False, out=None):
    """BatchNorm(+ReLU) backward of the Grad g through `layer` (the BNLayer of module bn), without a reduce pass when g brought its column sums -> (dc, dgamma, dbeta, dres):
    the gradient at the conv output (in `out` if given), the parameter gradients (in their bucket views where there are any), with want_dres the gated g as a tensor."""
    gg, gb = (grad_dst(bn.weight), grad_dst(bn.bias)) if need_w else (None, None)
    dc, dres, dgamma, dbeta = ops.bn_bwd(g.t, g.act, layer.c, layer.mean, layer.invstd, bn.weight, train=bn.training, want_dres=want_dres, mask=g.bits, out=out,
                                         sync_world=sync_world(bn), dgamma_out=gg, dbeta_out=gb, pre_partial=g.part)
    return dc, grad_alias(dgamma, gg), grad_alias(dbeta, gb), dres


def _bn_bwd2(g, layer1, bn1, layer2, bn2, need_w):
    """_bn_bwd for two BatchNorms whose outputs were added before one ReLU, in one sweep over g per pass (ops.bn_bwd2) -> (dc1, dgamma1, dbeta1), (dc2, dgamma2, dbeta2)."""
    o1, o2 = [(grad_dst(bn.weight), grad_dst(bn.bias)) if need_w else (None, None) for bn in (bn1, bn2)]
    dc1, dg1, db1, dc2, dg2, db2 = ops.bn_bwd2(g.t, g.bits, layer1.c, layer1.mean, layer1.invstd, bn1.weight, layer2.c, layer2.mean, layer2.invstd, bn2.weight, o1, o2,
                                               pre_partials=None if g.part is None else (g.part, g.part2))
    return (dc1, grad_alias(dg1, o1[0]), grad_alias(db1, o1[1])), (dc2, grad_alias(dg2, o2[0]), grad_alias(db2, o2[1]))


def _conv_wgrad(conv, x, dc, x2=None):
    """Weight gradient of conv on input x (x2: the second half of a virtual concat) from dc, the gradient at its output, written to its bucket view where there is one."""
    gw = grad_dst(conv.weight)
    return grad_alias(ops.conv2d_bwd_weight(x, dc, spec_of(conv), x2=x2, out=gw), gw)


def _conv_dgrad(dc, conv, x, below=None, addend=None, x2=None, prev=None, dx_half=False, addend_half=False):
    """Data gradient of conv on input x from dc, the gradient at its output: ONE launch, chosen by the first route that applies.  -> Grad.  The fused routes write a
    fresh dx from a single source; where the library does not serve the shape they return None and the plain form runs.
    below: (BNLayer, module) of the BatchNorm + ReLU that produced x.  In train mode, where the kernel has the staged store phase, its epilogue gates dx with those
    bits and emits that layer's column sums; otherwise the result carries the bits as its gate.
    addend: a Grad (tensor + optional bits gate) accumulated into dx by the epilogue.
    prev: the _BlockLink of the PREVIOUS bottleneck (bn3: its bn3 + output ReLU; bnd: its downsample BatchNorm behind the same ReLU, or None): dx, with its addend,
    which must be gated already, is that block's incoming gradient; where the pixel-stationary kernel serves the shape it is gated there and reduced against c3
    (and cd): the result carries that block's column sums."""
    spec, hw = spec_of(conv), x.shape[1:3]
    wb = prepared(conv.weight, dc.dtype)[1]
    add, add_bits = (addend.t, addend.bits) if addend is not None else (None, None)
    if dx_half:
        # a 1x1 stride-2 conv (a stage entry's downsample branch): its data gradient is non-zero at the even positions only -- return the DENSE gradient on the conv's own
        # output grid; the consumer adds it at the even positions (ops.conv2d_bwd_data_addend_half), the zero-filled tensor is never written
        return Grad(ops.conv2d_bwd_data(dc, wb, ConvSpec(spec.cin, spec.cout, 1, 1, 0, 1), dc.shape[1:3]))
    (lb, bnb), (l3, ld) = below or (None, None), (prev.bn3, prev.bnd) if prev is not None else (None, None)
    cross = l3 is not None and add is not None and add_bits is None and x2 is None
    r = None
    if addend_half:
        r = ops.conv2d_bwd_data_addend_half(dc, wb, spec, hw, add, None if l3 is None else (l3.bits, l3.c, l3.mean, l3.invstd))
    elif lb is not None and bnb.training and _BN_FUSE and add is None and x2 is None:
        r = ops.conv2d_bwd_data_bnstat(dc, wb, spec, hw, lb.bits, lb.c, lb.mean, lb.invstd)
    elif cross and ld is not None:        # the block in front is a stage's first one: bn3 + downsample BatchNorm behind its ReLU, both reduced here (the result has part2)
        r = ops.conv2d_bwd_data_addend_bnstat2(dc, wb, spec, hw, add, l3.bits, l3.c, l3.mean, l3.invstd, ld.c, ld.mean, ld.invstd)
    elif cross:
        r = ops.conv2d_bwd_data_addend_bnstat(dc, wb, spec, hw, add, l3.bits, l3.c, l3.mean, l3.invstd)
    if r is None:
        r = (ops.conv2d_bwd_data(dc, wb, spec, hw, addend=add, addend_mask=add_bits, C1=(x.shape[3] if x2 is not None else None)), None)
    return Grad(*r, bits=lb.bits if (lb is not None and r[1] is None) else None)            # the epilogue did not gate: the layer below's bits go with the result


# ------------------------------------------------------------------------------------------------ stem
class StemFn(torch.autograd.Function):
    """conv1 7x7 s2 -> bn1 -> relu -> maxpool 3x3 s2 (networks/backbones/resnet.py:124-125). img: NCHW float."""

    @staticmethod
    def forward(ctx, img, w, gamma, beta, net, dtype):
        bn = net.bn1
        c0, part = ops.stem_conv_fwd(img, w.detach(), dtype, bn.training)
        mean, invstd, scale, shift = _bn_coeffs(bn, part, c0.numel() // 64)
        pooled, idx = ops.stem_bn_relu_pool(c0, scale, shift, want_idx=True)
        ctx.net = net
        _save(ctx, img, BNLayer(c0, mean, invstd, None), idx, scale, shift)
        return pooled

    @staticmethod
    @once_differentiable
    def backward(ctx, dp):
        img, l0, idx, scale, shift = _saved(ctx)
        if _BN_FUSE:          # bn1's reduce pass rides in the pool / ReLU backward, which reads c0 anyway (round 5)
            g0, pp = ops.stem_pool_relu_bwd_bnstat(dp.contiguous(), idx, l0.c, scale, shift, l0.mean, l0.invstd)
        else:
            g0, pp = ops.stem_pool_relu_bwd(dp.contiguous(), idx, l0.c, scale, shift), None
        dc0, dgamma, dbeta, _ = _bn_bwd(Grad(g0, part=pp), l0, ctx.net.bn1, need_w=True)     # bn1's gradients are produced whether or not conv1's weight takes one
        dw = ops.stem_conv_bwd_weight(img, dc0) if ctx.needs_input_grad[1] else None
        return None, dw, dgamma, dbeta, None, None


class DeepStemFn(torch.autograd.Function):
    """conv1 3x3 s2 -> bn1 -> relu -> conv2 3x3 -> bn2 -> relu -> conv3 3x3 (64 -> 128) -> bn3 -> relu -> maxpool 3x3 s2
    (networks/backbones/resnet.py:144-153,187-190).  img: NCHW float; the result is NHWC [B, H/4, W/4, 128].
    conv1 and the pool are the stem kernels (csrc/stem3.hip, csrc/stem.hip); conv2 / conv3 are ordinary layers of the conv dispatch."""

    @staticmethod
    def forward(ctx, img, net, dtype, *params):
        bn1, bn2, bn3 = net.bn1, net.bn2, net.bn3
        w1 = net.conv1.weight.detach()
        wf3, _ = prepared(net.conv3.weight, dtype)
        if _frozen(ctx, bn1, bn2, bn3):
            # frozen statistics, nothing saved: bn1 + relu1 ride in conv1's launch, bn2 + relu2 in conv2's epilogue, bn3 + relu3 in the pool
            _, _, sc1, sh1 = _bn_eval_coeffs(bn1)
            a1, _ = ops.stem3_conv_fwd(img, w1, dtype, scale=sc1, shift=sh1)
            a2 = conv_bn_infer(a1, net.conv2, bn2, relu=True)
            c3, _ = ops.conv2d_fwd(a2, wf3, spec_of(net.conv3))
            _, _, sc3, sh3 = _bn_eval_coeffs(bn3)
            return ops.stem_bn_relu_pool_c(c3, sc3, sh3, want_idx=False)[0]
        c1, part = ops.stem3_conv_fwd(img, w1, dtype, want_stats=bn1.training)
        m1, i1, sc1, sh1 = _bn_coeffs(bn1, part, c1.numel() // 64)
        a1, k1 = ops.bn_act(c1, sc1, sh1, relu=True, want_mask=True)
        a2, l2 = conv_bn_fwd(a1, net.conv2, bn2, relu=True, want_mask=True)
        c3, part = ops.conv2d_fwd(a2, wf3, spec_of(net.conv3), want_stats=bn3.training)
        m3, i3, sc3, sh3 = _bn_coeffs(bn3, part, c3.numel() // c3.shape[-1])
        pooled, idx = ops.stem_bn_relu_pool_c(c3, sc3, sh3, want_idx=True)        # bn3 + relu3 + maxpool in one pass: relu3's output never exists
        ctx.net = net
        _save(ctx, img, BNLayer(c1, m1, i1, k1), a1, l2, a2, BNLayer(c3, m3, i3, None), idx, sc3, sh3)
        return pooled

    @staticmethod
    @once_differentiable
    def backward(ctx, dp):
        img, l1, a1, l2, a2, l3, idx, sc3, sh3 = _saved(ctx)
        net = ctx.net
        need_w = ctx.needs_input_grad[3]            # the stem's parameters are all-or-nothing frozen, like a bottleneck's
        # pool + relu3 backward with bn3's column sums in the same sweep over c3; conv3's and conv2's data gradients gate with the ReLU bits below and
        # emit the next BatchNorm's column sums where their kernel has the staged store phase (_conv_dgrad: below)
        g3, p3 = ops.stem_pool_relu_bwd_bnstat_c(dp.contiguous(), idx, l3.c, sc3, sh3, l3.mean, l3.invstd)
        dc3, dg3, db3, _ = _bn_bwd(Grad(g3, part=p3), l3, net.bn3, need_w)
        dw3 = _conv_wgrad(net.conv3, a2, dc3) if need_w else None
        da2 = _conv_dgrad(dc3, net.conv3, a2, below=(l2, net.bn2))
        dc2, dg2, db2, _ = _bn_bwd(da2, l2, net.bn2, need_w)
        dw2 = _conv_wgrad(net.conv2, a1, dc2) if need_w else None
        da1 = _conv_dgrad(dc2, net.conv2, a1, below=(l1, net.bn1))
        dc1, dg1, db1, _ = _bn_bwd(da1, l1, net.bn1, need_w)
        gw = grad_dst(net.conv1.weight) if need_w else None
        dw1 = grad_alias(ops.stem3_conv_bwd_weight(img, dc1, out=gw), gw) if need_w else None        # the image needs no data gradient
        return (None, None, None, dw1, dg1, db1, dw2, dg2, db2, dw3, dg3, db3)


def deep_stem_params(net):
    return [net.conv1.weight, net.bn1.weight, net.bn1.bias, net.conv2.weight, net.bn2.weight, net.bn2.bias, net.conv3.weight, net.bn3.weight, net.bn3.bias]


# ------------------------------------------------------------------------------------------------ bottleneck
class _BlockLink:
    """What two consecutive bottlenecks of ONE forward pass hand each other for the cross-block bn3 fusion (_BN_CROSS).  The producer's forward makes it
    (bn3: the BNLayer of its output BatchNorm + ReLU; bnd: that of the downsample BatchNorm behind the same ReLU, a stage's first block; out_ptr / out_shape: the
    tensor it returned), the consumer's forward picks it up from the producer module -- checked against its own input -- and keeps it in its ctx; the consumer's
    backward leaves the Grad its conv1 data-gradient epilogue produced (the gradient tensor with the column sums that belong to it) in pre3, the producer's
    backward takes it.  Nothing is read from module state at backward time.  pre3 holds the gradient tensor itself, not its address (an address can be reused):
    where the producer's backward never runs, the tensor lives until the producer module's next forward drops the link."""
    __slots__ = ('bn3', 'bnd', 'pre3', 'out_ptr', 'out_shape')

    def __init__(self):
        self.bn3 = self.bnd = self.pre3 = self.out_ptr = self.out_shape = None


class BottleneckFn(torch.autograd.Function):
    """networks/backbones/resnet.py:57-78 as one kernel chain; x and the result are NHWC."""

    @staticmethod
    def forward(ctx, x, blk, *params):
        bns = [blk.bn1, blk.bn2, blk.bn3] + ([blk.downsample[1]] if blk.downsample is not None else [])
        # the hand-over record of the block that produced x IN THIS FORWARD PASS (a second forward before the first backward makes new records:
        # a backward never sees another pass's ReLU bits or column sums)
        pm = blk.__dict__.get('_sl_prev')
        plink = pm.__dict__.get('_sl_link') if pm is not None else None
        ctx.prev_link = plink if (plink is not None and plink.out_ptr == x.data_ptr() and plink.out_shape == tuple(x.shape)) else None
        blk.__dict__['_sl_link'] = None
        if _frozen(ctx, *bns):
            a1 = conv_bn_infer(x, blk.conv1, blk.bn1, relu=True)
            a2 = conv_bn_infer(a1, blk.conv2, blk.bn2, relu=True)
            res = x if blk.downsample is None else conv_bn_infer(x, blk.downsample[0], blk.downsample[1], relu=False)
            return conv_bn_infer(a2, blk.conv3, blk.bn3, relu=blk.last_relu, residual=res)
        a1, l1 = conv_bn_fwd(x, blk.conv1, blk.bn1, relu=True, want_mask=True)
        a2, l2 = conv_bn_fwd(a1, blk.conv2, blk.bn2, relu=True, want_mask=True)
        dsc, dbn = (blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else (None, None)
        if dsc is not None and _BN_DUAL_FWD and blk.bn3.training and dbn.training and not sync_world(blk.bn3) and not sync_world(dbn) and a2.dtype == x.dtype:
            # a stage's first block: the downsample BatchNorm is applied inside bn3's pass (ops.bn_act2), its normalised output is never written
            cd, part = ops.conv2d_fwd(x, prepared(dsc.weight, x.dtype)[0], spec_of(dsc), want_stats=True)
            md, isd, scd, shd = _bn_coeffs(dbn, part, cd.numel() // cd.shape[-1])
            c3, part = ops.conv2d_fwd(a2, prepared(blk.conv3.weight, a2.dtype)[0], spec_of(blk.conv3), want_stats=True)
            m3, is3, sc3, sh3 = _bn_coeffs(blk.bn3, part, c3.numel() // c3.shape[-1])
            out, k3 = ops.bn_act2(c3, sc3, sh3, cd, scd, shd, relu=blk.last_relu, want_mask=True)
            ld, l3 = BNLayer(cd, md, isd, None), BNLayer(c3, m3, is3, k3)
        else:
            res, ld = conv_bn_fwd(x, dsc, dbn, relu=False) if dsc is not None else (x, None)
            out, l3 = conv_bn_fwd(a2, blk.conv3, blk.bn3, relu=blk.last_relu, residual=res, want_mask=True)
        ctx.blk = blk
        ctx.has_ds = blk.downsample is not None
        # the next bottleneck's backward produces this block's incoming gradient: it may gate it and reduce it against c3 right there (_BN_CROSS)
        link = ctx.link = blk.__dict__['_sl_link'] = _BlockLink()
        dual_ok = ctx.has_ds and _BN_DUAL and blk.downsample[1].training and not sync_world(blk.bn3)      # the consumer's one-sweep dual backward (ops.bn_bwd2) must apply
        link.bn3 = l3 if (_BN_CROSS and l3.bits is not None and blk.bn3.training and (not ctx.has_ds or dual_ok) and any(ctx.needs_input_grad)) else None
        link.bnd = ld if (link.bn3 is not None and ctx.has_ds) else None
        link.out_ptr, link.out_shape = out.data_ptr(), tuple(out.shape)
        _save(ctx, x, l1, a1, l2, a2, l3, ld)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        blk = ctx.blk
        x, l1, a1, l2, a2, l3, ld = _saved(ctx)       # l3.bits: ReLU bits of the block output (they gate BOTH the bn3 and the shortcut gradient)
        dout = dout.contiguous()
        need_w = ctx.needs_input_grad[2]            # params are all-or-nothing frozen in this model family
        need_x = ctx.needs_input_grad[0]
        # bn3 and the downsample BN sit behind the same ReLU: one sweep over dout and its bits for both reduces, one for both applies (ops.bn_bwd2)
        dual = ctx.has_ds and _BN_DUAL and l3.bits is not None and blk.bn3.training and blk.downsample[1].training and not sync_world(blk.bn3)
        # this block's incoming gradient may have been gated and reduced against c3 by the block behind it (its conv1 data gradient epilogue): the tensor
        # autograd hands over must be exactly the one that epilogue wrote (a second consumer of this block's output would have made autograd sum into a new one)
        link = ctx.link
        pre3, link.pre3, link.bn3, link.bnd = link.pre3, None, None, None
        g3 = Grad(dout, bits=l3.bits)
        # (one set of column sums serves a block with an identity shortcut; a pair, from the dual store loop of the block behind, bn3 AND the downsample BatchNorm)
        if pre3 is not None and pre3.t.data_ptr() == dout.data_ptr() and pre3.t.shape == dout.shape and (dual if pre3.part2 is not None else not ctx.has_ds):
            g3 = pre3                                # dout is gated already: no bits for bn3, none for the identity shortcut
        dres = None
        if dual:
            (dc3, dg3, db3), (dcd, dgd, dbd) = _bn_bwd2(g3, l3, blk.bn3, ld, blk.downsample[1], need_w)
        # the block in front of this one can take its bn3 column sums from this block's conv1 data gradient only if the shortcut gradient enters that epilogue
        # gated already: either dout arrived gated (g3.part), or the shortcut is a downsample branch, or -- the start of a chain inside a stage -- bn3's apply pass
        # also writes the gated gradient (one extra write of dout's size, repaid by every block further up the stage)
        prev = ctx.prev_link if (need_x and _BN_CROSS) else None
        if prev is not None and (prev.bn3 is None or prev.bn3.c.shape != x.shape or prev.bn3.c.dtype != x.dtype
                                 or not ops.conv2d_bwd_data_addend_bnstat_ok(x, spec_of(blk.conv1))):
            prev = None
        if not dual:
            dc3, dg3, db3, dres = _bn_bwd(g3, l3, blk.bn3, need_w, want_dres=prev is not None and not ctx.has_ds and g3.bits is not None)
        # the data gradients of conv3 and conv2 gate their result with the ReLU bits of the layer below and emit its BN-backward column sums in the epilogue
        # (where the kernel has the staged store phase: layer3 / layer4 at the bench shapes): that layer's reduce pass over (g, c) disappears
        dw3 = _conv_wgrad(blk.conv3, a2, dc3) if need_w else None
        da2 = _conv_dgrad(dc3, blk.conv3, a2, below=(l2, blk.bn2))
        dc2, dg2, db2, _ = _bn_bwd(da2, l2, blk.bn2, need_w)
        dw2 = _conv_wgrad(blk.conv2, a1, dc2) if need_w else None
        da1 = _conv_dgrad(dc2, blk.conv2, a1, below=(l1, blk.bn1))
        grads_ds, half = (), False
        if ctx.has_ds:
            dsc = blk.downsample[0]
            half = (_DS_HALF and need_x and dsc.kernel_size == (1, 1) and dsc.stride == (2, 2) and dsc.padding == (0, 0) and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0
                    and ops.conv2d_bwd_data_addend_half_ok(x, spec_of(blk.conv1)))
            if not dual:
                dcd, dgd, dbd, _ = _bn_bwd(g3, ld, blk.downsample[1], need_w)
            dwd = _conv_wgrad(dsc, x, dcd) if need_w else None
            shortcut = _conv_dgrad(dcd, dsc, x, dx_half=half) if need_x else None
            grads_ds = (dwd, dgd, dbd)
        elif dres is not None:
            shortcut = Grad(dres)                   # identity shortcut, gated by bn3's apply pass (chain start, see above)
        else:
            shortcut = Grad(dout, bits=g3.bits)     # identity shortcut: dout * relu'(out), gated inside the dgrad epilogue (no bits: dout arrived gated, or no ReLU)
        if shortcut is not None and shortcut.bits is not None:
            prev = None
        dc1, dg1, db1, _ = _bn_bwd(da1, l1, blk.bn1, need_w)
        dw1 = _conv_wgrad(blk.conv1, x, dc1) if need_w else None
        gx = _conv_dgrad(dc1, blk.conv1, x, addend=shortcut, prev=prev, addend_half=half) if need_x else None
        if prev is not None and gx.part is not None:            # (prev is None where need_x is false)
            prev.pre3 = gx
        return (gx.t if need_x else None, None, dw1, dg1, db1, dw2, dg2, db2, dw3, dg3, db3) + grads_ds


def bottleneck_params(blk):
    p = [blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, blk.conv2.weight, blk.bn2.weight, blk.bn2.bias,
         blk.conv3.weight, blk.bn3.weight, blk.bn3.bias]
    if blk.downsample is not None:
        p += [blk.downsample[0].weight, blk.downsample[1].weight, blk.downsample[1].bias]
    return p


# ------------------------------------------------------------------------------------------------ pyramid pooling
# How a decoder describes the stages of its pyramid (per level: adaptive pool -> 1x1 conv -> BatchNorm -> ReLU) to stages_fwd / stages_bwd; made per call, so the hooks are
# read when the chain runs.  sizes / convs / bns: per level; pitch: channels of a pyramid row; w_fwd() / w_dgrad(): the stage weights in ops.ppm_rows_gemm's forward and
# data-gradient form; coeffs(bn, c, part, count) -> (mean, invstd, scale, shift) of a level; gamma(bn): its scale vector at the pitch; dst(p): where parameter p's gradient is to
# be written (None: a fresh tensor) and w_dsts(): that of all stage conv weights; grad(t, dst, p): what the backward returns for p's gradient t, which the kernels wrote at the
# pitch; bn_grouped(call) / wgrad_grouped(bn_grouped): all levels' BatchNorm + ReLU backward in ONE launch (ops.ppm_stage_bn_bwd) / all stage weight gradients in one launch
# (ops.ppm_rows_wgrad, which needs the gradient at every level's conv output complete).
Pyramid = namedtuple('Pyramid', 'sizes convs bns pitch w_fwd w_dgrad coeffs gamma dst w_dsts grad bn_grouped wgrad_grouped')


def ppm_stages(dec):
    """The PSPNet-POP pyramid (pspnet_pop.PSPModule): the levels' prepared float weights, gradients written into DDP's bucket views where there are any; the grouped BatchNorm
    backward saves twelve latency-bound launches per step (round 5), SyncBatchNorm stages take the per-level chain."""
    convs, bns = [st[1] for st in dec.stages], [st[2] for st in dec.stages]
    return Pyramid(dec.sizes, convs, bns, pitch=convs[0].out_channels, w_fwd=lambda: _stage_weights(dec)[0], w_dgrad=lambda: _stage_weights(dec)[1],
                   coeffs=lambda bn, c, part, count: _bn_coeffs(bn, part, count), gamma=lambda bn: bn.weight,
                   dst=grad_dst, w_dsts=lambda: [grad_dst(c.weight) for c in convs], grad=lambda t, dst, p: grad_alias(t if t is dst else t.view_as(p), dst),
                   bn_grouped=lambda call: bool(_BN_FUSE and _STAGE_BN_GROUPED and call.numel() and not any(sync_world(bn) for bn in bns)),
                   wgrad_grouped=lambda bn_grouped: _PPM_WGRAD_GROUPED and bn_grouped)


def _level_rows(B, sizes):
    """Row range [off[k], off[k + 1]) of level k in the pyramid's row tensors."""
    off = [0]
    for s in sizes:
        off.append(off[-1] + B * s * s)
    return off


def stages_fwd(d, x, frozen=False, after_level=None):
    """The stages of pyramid d on the NHWC map x: adaptive pool, the four 1x1 convs as ONE grouped skinny GEMM over the pyramid rows (16..576 rows per level), per level
    BatchNorm + ReLU -> StageRec.  The stage path is fp32 (see ppm.hip).  frozen: a call that keeps nothing and takes no batch statistics; after_level(k, act): called
    right after level k's activation rows are written."""
    B, sizes = x.shape[0], d.sizes
    pooled = ops.ppm_pool_fwd(x, sizes)
    call, part = ops.ppm_rows_gemm(pooled, d.w_fwd(), B, sizes, want_stats=any(bn.training for bn in d.bns))
    stage_act = torch.empty_like(call)
    off, grp = _level_rows(B, sizes), None if frozen else ops.ppm_stat_groups(B, sizes)
    ml, il = [], []
    for k, bn in enumerate(d.bns):
        c, act = call[off[k]:off[k + 1]], stage_act[off[k]:off[k + 1]]
        m, i, scale, shift = d.coeffs(bn, c, part[grp[k]:grp[k + 1]] if bn.training else None, off[k + 1] - off[k])
        ops.bn_act(c, scale, shift, relu=True, out=act)
        if after_level is not None:
            after_level(k, act)
        ml.append(m); il.append(i)
    return StageRec(pooled, call, stage_act, ml, il)


def stages_bwd(d, rec, dstage, x_shape, x_dtype, need_w, need_x, dcat, cat_off):
    """Backward of stages_fwd from dstage, the gradient at the activation rows: BatchNorm + ReLU backward and the stage convs' weight gradients, each grouped or level by
    level as d says, the row GEMM back to the pooled rows and the pool backward, which adds the feature map's share dcat[..., cat_off:] of the concat's gradient.
    -> (dx or None, [d conv weight, d gamma, d beta] per level)."""
    B, sizes, nl = x_shape[0], d.sizes, len(d.sizes)
    pooled, call, stage_act, ml, il = rec
    P, Cf, off = call.shape[1], pooled.shape[1], _level_rows(B, sizes)
    dc_all = torch.empty_like(stage_act)
    vdst = [(d.dst(bn.weight), d.dst(bn.bias)) if need_w else (None, None) for bn in d.bns]
    wdst = d.w_dsts() if need_w else None
    grouped = d.bn_grouped(call)
    if grouped:
        tmp = torch.empty((nl, 2, P), dtype=torch.float32, device=call.device)
        dgl, dbl = [[v[j] if v[j] is not None else tmp[k, j] for k, v in enumerate(vdst)] for j in (0, 1)]
        ops.ppm_stage_bn_bwd(dstage, stage_act, call, B, sizes, ml, il, [d.gamma(bn) for bn in d.bns], [bn.training for bn in d.bns], dgl, dbl, out=dc_all)
    dws_all = ops.ppm_rows_wgrad(dc_all, pooled, B, sizes, outs=wdst) if (need_w and d.wgrad_grouped(grouped)) else None
    grads = []
    for k, (s, conv, bn) in enumerate(zip(sizes, d.convs, d.bns)):
        rows = slice(off[k], off[k + 1])
        if grouped:
            dgs, dbs = dgl[k], dbl[k]
        else:
            _, _, dgs, dbs = ops.bn_bwd(dstage[rows], stage_act[rows], call[rows], ml[k], il[k], d.gamma(bn), train=bn.training, out=dc_all[rows],
                                        sync_world=sync_world(bn), dgamma_out=vdst[k][0], dbeta_out=vdst[k][1])
        if not need_w:
            grads += [None, None, None]
            continue
        gws = wdst[k] if wdst is not None else None
        dws = dws_all[k] if dws_all is not None else ops.conv2d_bwd_weight(pooled[rows].view(B, s, s, Cf), dc_all[rows].view(B, s, s, P), ConvSpec(Cf, P, 1), out=gws)
        grads += [d.grad(dws, gws, conv.weight), d.grad(dgs, vdst[k][0], bn.weight), d.grad(dbs, vdst[k][1], bn.bias)]
    dx = None
    if need_x:
        dpooled = ops.ppm_rows_gemm(dc_all, d.w_dgrad(), B, sizes)[0]
        dx = ops.ppm_pool_bwd(dpooled, x_shape, x_dtype, sizes, dcat=dcat, cat_off=cat_off)
    return dx, grads


class PPMFn(torch.autograd.Function):
    """networks/pspnet_pop.py:31-35: 4 x (adaptive pool -> 1x1 -> BN -> ReLU -> bilinear up) (+) feats -> 3x3 -> BN -> ReLU -> 1x1+bias.
    The 4096-channel concat is virtual: the 3x3 conv reads [priors | feats] from two tensors."""

    @staticmethod
    def forward(ctx, x4, dec, *params):
        sizes, bt = dec.sizes, dec.bottleneck
        B, H, W, Cf = x4.shape
        frozen = _frozen(ctx, bt[1], *[st[2] for st in dec.stages])
        rec = stages_fwd(ppm_stages(dec), x4, frozen)
        fact, priors, lb = _PPM_FACTORISED, None, None
        if fact:
            # the prior half of the 3x3 conv contracted on the s x s grids (exact; see ppm.hip), the x4 half on the MFMA kernel with the gathered prior term entering
            # before the BatchNorm -- half the FLOPs of the virtual-concat conv, and a shape the patch kernel serves
            N = bt[0].out_channels
            wq_f, _, wf4, _ = _ppm_weights(bt[0].weight, rec.stage_act.shape[1], len(sizes), x4.dtype)
            q, _ = ops.ppm_rows_gemm(rec.stage_act, wq_f, B, sizes)
            gpri = ops.ppm_fact_gather(q, x4.shape, sizes, N, x4.dtype)
            spec4 = ConvSpec(Cf, N, 3, 1, 1, 1)
        else:
            priors = ops.ppm_upsample_fwd(rec.stage_act, x4.shape, sizes, x4.dtype)
        if frozen and fact:
            _, _, scale, shift = _bn_eval_coeffs(bt[1])
            ab = ops.conv2d_affine_fwd(x4, wf4, spec4, scale, shift, relu=True, pre_addend=gpri)
        elif frozen:
            ab = conv_bn_infer(priors, bt[0], bt[1], relu=True, x2=x4)
        elif fact:
            cb, part = ops.conv2d_fwd(x4, wf4, spec4, pre_addend=gpri, want_stats=bt[1].training)
            mb, ib, scale, shift = _bn_coeffs(bt[1], part, cb.numel() // N)
            ab, kb = ops.bn_act(cb, scale, shift, relu=True, want_mask=True)
            lb = BNLayer(cb, mb, ib, kb)
        else:
            ab, lb = conv_bn_fwd(priors, bt[0], bt[1], relu=True, x2=x4)          # no ReLU bits: the backward gates with ab itself
        wf, _ = prepared(bt[3].weight, x4.dtype)
        feat, _ = ops.conv2d_fwd(ab, wf, spec_of(bt[3]), bias=bt[3].bias.detach())
        if not frozen:
            ctx.dec, ctx.fact = dec, fact
            _save(ctx, x4, rec, priors, lb, ab)
        return feat

    @staticmethod
    @once_differentiable
    def backward(ctx, dfeat):
        dec = ctx.dec
        sizes, nl = dec.sizes, len(dec.sizes)
        x4, rec, priors, lb, ab = _saved(ctx)      # lb.bits: ReLU bits of the bottleneck BatchNorm (factorised path)
        stage_act = rec.stage_act
        B, H, W, Cf = x4.shape
        Cs = stage_act.shape[1]
        bt = dec.bottleneck
        dfeat = dfeat.contiguous()
        need_w = ctx.needs_input_grad[2]
        need_x = ctx.needs_input_grad[0]
        # the classifier conv's data gradient gates its result with the bottleneck ReLU's bits and emits the bottleneck BatchNorm's backward column sums
        # in its epilogue where the kernel serves the shape (round 5: one 36 us reduce pass less per step)
        if ctx.fact:
            dab = _conv_dgrad(dfeat, bt[3], ab, below=(lb, bt[1]))
        else:                 # direct path: no bits were kept, the activation itself is the gate
            dab = Grad(ops.conv2d_bwd_data(dfeat, prepared(bt[3].weight, x4.dtype)[1], spec_of(bt[3]), (H, W)), act=ab)
        gwf = grad_dst(bt[3].weight) if need_w else None
        dwf = dbias = None
        if need_w:
            # weight + bias gradient of the biased 1x1 conv in one kernel (the bias column sums come out of the weight-gradient kernel's dy fragments: round 6, one pass over dfeat less)
            dwf, dbias = ops.conv2d_bwd_weight_bias(ab, dfeat, spec_of(bt[3]), out=gwf)
            dwf = grad_alias(dwf, gwf)
        if ctx.fact:
            N = bt[0].out_channels
            wq_f, wq_b, wf4, wb4 = _ppm_weights(bt[0].weight, Cs, nl, x4.dtype)
            dcb, dgb, dbb, _ = _bn_bwd(dab, lb, bt[1], need_w)
            spec4 = ConvSpec(Cf, N, 3, 1, 1, 1)
            dcat = ops.conv2d_bwd_data(dcb, wb4, spec4, (H, W))                     # gradient of the x4 half only: [B,H,W,Cf]
            cat_off = 0
            dwb = None
            gq = ops.ppm_fact_scatter(dcb, x4.shape, sizes)
            dstage, _ = ops.ppm_rows_gemm(gq, wq_b, B, sizes)
            if need_w:
                gwb = grad_dst(bt[0].weight)
                dwb = gwb if gwb is not None else torch.empty_like(bt[0].weight, dtype=torch.float32)
                ops.conv2d_bwd_weight(x4, dcb, spec4, out=dwb, out_ci_off=nl * Cs)
                dwq = torch.empty((nl, 9 * N, Cs), dtype=torch.float32, device=x4.device)
                if _PPM_WGRAD_GROUPED:
                    ops.ppm_rows_wgrad(gq, stage_act, B, sizes, outs=[dwq[k] for k in range(nl)])      # all levels in one launch (round 6)
                else:
                    qspec, off = ConvSpec(Cs, 9 * N, 1), 0
                    for k, s in enumerate(sizes):
                        n = B * s * s
                        ops.conv2d_bwd_weight(stage_act[off:off + n].view(B, s, s, Cs), gq[off:off + n].view(B, s, s, 9 * N), qspec,
                                              out=dwq[k].view(9 * N, Cs, 1, 1))
                        off += n
                ops.ppm_dwq_scatter(dwq, dwb, Cs, nl)
                dwb = grad_alias(dwb, gwb)
        else:
            dcb, dgb, dbb, _ = _bn_bwd(dab, lb, bt[1], need_w)
            dwb = _conv_wgrad(bt[0], priors, dcb, x2=x4) if need_w else None
            dcat = _conv_dgrad(dcb, bt[0], priors, x2=x4).t
            dstage = ops.ppm_upsample_bwd(dcat, x4.shape, sizes, Cs)
            cat_off = len(sizes) * Cs
        dx4, gstage = stages_bwd(ppm_stages(dec), rec, dstage, x4.shape, x4.dtype, need_w, need_x, dcat, cat_off)
        return (dx4, None, *gstage, dwb, dgb, dbb, dwf, dbias)


def set_ppm_factorised(flag):
    """Test hook: choose between the factorised prior path (default) and the direct virtual-concat 3x3 conv."""
    global _PPM_FACTORISED
    _PPM_FACTORISED = bool(flag)


def _stage_weights(dec):
    """The stage 1x1 weights for the grouped GEMMs: (per level [Cs][Cf] forward, per level [Cf][Cs] data gradient) -- the float copies weight preparation makes anyway
    (refresh_weights: the stage convs are in the plan with float32), handed to ops.ppm_rows_gemm as per-level pointers.  (Until round 6 they were stacked and transposed
    with two torch launches per step: 37 us.)"""
    fs, bs = [], []
    for st in dec.stages:
        wf, wb = prepared(st[1].weight, torch.float32)
        fs.append(wf); bs.append(wb)
    return fs, bs


def _ppm_weights(w, Cs, nl, dtype):
    """Per-level 1x1 weights of the factorised prior path (float) + GEMM layouts of the x4 channel slice, cached on the Parameter."""
    ent = getattr(w, '_sl_ppm', None)
    if ent is None or ent[0] != _wver(w) or ent[1] != dtype or ent[2] != w.data_ptr():
        wq_f, wq_b = ops.ppm_wq_prep(w, Cs, nl)
        wf4, wb4 = ops.weight_prep_slice(w, dtype, nl * Cs, w.shape[1] - nl * Cs)
        ent = (_wver(w), dtype, w.data_ptr(), wq_f, wq_b, wf4, wb4)
        w._sl_ppm = ent
    return ent[3], ent[4], ent[5], ent[6]


def ppm_params(dec):
    p = []
    for st in dec.stages:
        p += [st[1].weight, st[2].weight, st[2].bias]
    bt = dec.bottleneck
    return p + [bt[0].weight, bt[1].weight, bt[1].bias, bt[3].weight, bt[3].bias]


# ------------------------------------------------------------------------------------------------ POP head
def _row_parts(R, big):
    """Row ranges the MLP GEMMs run on: the pixel rows (a multiple of 256: whole 256-row tiles, ONE round of the persistent tile kernel on 256 CUs) and the
    handful of prototype rows behind them as a launch of their own -- in one launch 65 536 + 14 rows are 257 tiles, i.e. a second round for 14 rows (measured: the
    512 -> 512 GEMMs of the head ran at 375 TFLOP/s, half of what the same kernel reaches on 65 536 rows)."""
    if big and 0 < big < R and big % 256 == 0 and big >= 256 * 96:
        return [(0, big), (big, R)]
    return [(0, R)]


def _mlp_fwd(X, cls, big=0):
    """classifier MLP (pspnet_pop.py:46-52) on rows X [R,512]: two MFMA 1x1 convs with fused ReLU, then a row dot.  big: number of leading pixel rows (see _row_parts)."""
    R, Cn = X.shape
    w1f, _ = prepared(cls[0].weight, X.dtype)
    w2f, _ = prepared(cls[2].weight, X.dtype)
    h1, h2 = torch.empty_like(X), torch.empty_like(X)
    for a, b in _row_parts(R, big):
        ops.conv2d_fwd(X[a:b].view(1, 1, b - a, Cn), w1f, spec_of(cls[0]), relu=True, out=h1[a:b].view(1, 1, b - a, Cn))
        ops.conv2d_fwd(h1[a:b].view(1, 1, b - a, Cn), w2f, spec_of(cls[2]), relu=True, out=h2[a:b].view(1, 1, b - a, Cn))
    w3 = cls[4].weight.detach().view(-1)
    z = ops.rowdot_fwd(h2, w3)
    return h1.view(1, 1, R, Cn), h2.view(1, 1, R, Cn), z


def _mlp_bwd(X, h1, h2, cls, dz, need_w, need_x, big=0):
    R, Cn = X.shape
    w3 = cls[4].weight.detach().view(-1)
    dh2, dw3 = ops.rowdot_bwd(h2.view(R, Cn), w3, dz)
    h1r = h1.view(R, Cn)
    _, w2b = prepared(cls[2].weight, X.dtype)
    dh1 = torch.empty_like(dh2)
    parts = _row_parts(R, big)
    for a, b in parts:
        ops.conv2d_bwd_data(dh2[a:b].view(1, 1, b - a, Cn), w2b, spec_of(cls[2]), (1, b - a), mask_src=h1r[a:b].view(1, 1, b - a, Cn), out=dh1[a:b].view(1, 1, b - a, Cn))
    dh2, dh1 = dh2.view(1, 1, R, Cn), dh1.view(1, 1, R, Cn)
    g2 = grad_dst(cls[2].weight) if need_w else None
    dw2 = grad_alias(ops.conv2d_bwd_weight(h1, dh2, spec_of(cls[2]), out=g2), g2) if need_w else None
    dX = None
    if need_x:
        _, w1b = prepared(cls[0].weight, X.dtype)
        dX = torch.empty_like(X)
        for a, b in parts:
            ops.conv2d_bwd_data(dh1[0, 0, a:b].view(1, 1, b - a, Cn), w1b, spec_of(cls[0]), (1, b - a), out=dX[a:b].view(1, 1, b - a, Cn))
    g1 = grad_dst(cls[0].weight) if need_w else None
    dw1 = grad_alias(ops.conv2d_bwd_weight(X.view(1, 1, R, Cn), dh1, spec_of(cls[0]), out=g1), g1) if need_w else None
    return dX, dw1, dw2, (dw3.view_as(cls[4].weight) if need_w else None)


def _base_chain(model, S_b, dtype, frozen):
    """ft mode: the base classifier over the +-base prototype rows (pspnet_pop.py:210-216).  With the base prototypes and the base classifier frozen (ft_pop.py:197-203)
    its result is the same every iteration: kept on the model, keyed on the versions of what it is computed from (four launches per step less).  Never created while a
    graph is being captured (its tensors would live in the graph's pool)."""
    def run():
        Xb = torch.empty((2 * S_b.shape[0], S_b.shape[1]), dtype=dtype, device=S_b.device)
        ops.pop_proto_rows(S_b.contiguous(), Xb)
        return (Xb,) + tuple(_mlp_fwd(Xb, model.classifier))
    key = base_chain_key(model) if frozen else None
    if key is None:
        return run()
    key = key + (dtype, tuple(S_b.shape))
    ent = model.__dict__.get('_sl_base_chain')
    if ent is not None and ent[0] == key:
        return ent[1]
    out = run()
    if not (S_b.is_cuda and torch.cuda.is_current_stream_capturing()):
        model.__dict__['_sl_base_chain'] = (key, out)
    return out


def unwrapped(model):
    """The module behind any `.module` wrappers (engine.ModuleWrapper, bucket_step.BucketedReplica, nn.DataParallel / DistributedDataParallel): the one that owns
    `base_emb`, `classifier` and the `_sl_base_chain` entry."""
    while getattr(model, 'module', None) is not None:
        model = model.module
    return model


def base_chain_key(model):
    """What the cached rows of _base_chain are computed from (versions + addresses of the frozen base classifier's weights and of base_emb), or None when the cache does
    not apply.  The step graphs put it into their state key (graph_step.StepLifecycle): a captured fine-tune step has the cached tensors baked in, so a change of these
    weights behind a graph (load_state_dict, init_cls_n) must force a re-capture -- every other weight is picked up through its pointer, these rows are not (round-5
    advisor).  `model` may be wrapped: the drivers hand the step graphs what engine.data_parallel returned."""
    model = unwrapped(model)
    emb = getattr(model, 'base_emb', None)
    cls = getattr(model, 'classifier', None)
    if not (_BASE_CHAIN_CACHE and getattr(model, 'is_ft', False) and emb is not None and cls is not None and not emb.requires_grad):
        return None
    ws = cls_params(cls)
    if any(w.requires_grad for w in ws):
        return None
    return (tuple((_wver(w), w.data_ptr()) for w in ws), emb._version, emb.data_ptr())


class PopHeadFn(torch.autograd.Function):
    """orthogonal_decompose + classifier(s) in the collapsed form.
    feat NHWC [B,h,w,512]; S_b / S_n: L2-normalised prototypes (float).  Returns preds [B, 1+Kb+Kn, h, w] float,
    channel order [bg | base | novel] (pspnet_pop.py:159,219).
    Base mode (cls_n is None): one MLP chain (classifier) over [bg rows ; +-S_b].
    ft mode: classifier over [+-S_b] (base scalars), classifier_n over [bg rows ; +-S_n]."""

    @staticmethod
    def forward(ctx, feat, S_b, S_n, model, *params):
        B, h, w, Cn = feat.shape
        R, N = B * h * w, h * w
        Kb = S_b.shape[0]
        Kn = 0 if S_n is None else S_n.shape[0]
        ft = S_n is not None
        S = torch.cat([S_b, S_n], 0).contiguous() if ft else S_b.contiguous()
        feats2d = feat.view(R, Cn)
        S_main = S_n.contiguous() if ft else S            # prototypes whose +- rows ride the bg chain
        Km = S_main.shape[0]
        X = torch.empty((R + 2 * Km, Cn), dtype=feat.dtype, device=feat.device)
        proj = ops.pop_decompose_into(feats2d, S, X[:R])
        ops.pop_proto_rows(S_main, X[R:])
        cls_main = model.classifier_n if ft else model.classifier
        h1, h2, z = _mlp_fwd(X, cls_main, big=R)
        if ft:
            Xb, h1b, h2b, zb = _base_chain(model, S_b, feat.dtype, frozen=not (ctx.needs_input_grad[1] or ctx.needs_input_grad[4]))
            a = torch.cat([zb[:Kb], z[R:R + Kn]]).contiguous()
            b = torch.cat([zb[Kb:], z[R + Kn:]]).contiguous()
        else:
            Xb = h1b = h2b = None
            a, b = z[R:R + Kb].contiguous(), z[R + Kb:].contiguous()
        z_bg = z[:R].contiguous()
        preds = ops.pop_combine_fwd(proj, z_bg, a, b, B, N)
        ctx.model, ctx.ft, ctx.dims = model, ft, (B, h, w, Cn, Kb, Kn)
        ctx.save_for_backward(feat, S, X, proj, h1, h2, a, b, *([Xb, h1b, h2b] if ft else []))
        return preds.view(B, 1 + Kb + Kn, h, w)

    @staticmethod
    @once_differentiable
    def backward(ctx, dpreds):
        model, ft = ctx.model, ctx.ft
        B, h, w, Cn, Kb, Kn = ctx.dims
        R, N = B * h * w, h * w
        sv = ctx.saved_tensors
        feat, S, X, proj, h1, h2, a, b = sv[:8]
        ni = ctx.needs_input_grad
        need_feat, need_sb, need_sn = ni[0], ni[1], ni[2]
        dpreds = dpreds.contiguous().view(B, 1 + Kb + Kn, N)
        dz_bg, dproj, da, db = ops.pop_combine_bwd(dpreds, proj, a, b, B, N)
        cls_main = model.classifier_n if ft else model.classifier
        npar = 3
        need_w_main = ni[4 + (npar if ft else 0)]
        if ft:
            dz = torch.cat([dz_bg, da[Kb:], db[Kb:]]).contiguous()
        else:
            dz = torch.cat([dz_bg, da, db]).contiguous()
        dX, dw1, dw2, dw3 = _mlp_bwd(X, h1, h2, cls_main, dz, need_w_main, need_feat or need_sb or need_sn, big=R)
        gb = (None, None, None)
        dS = None
        dfeat = None
        if need_feat or need_sb or need_sn:
            dq, dS = ops.pop_decompose_bwd(dX[:R], feat.view(R, Cn), S, proj, dproj)
            dfeat = dq.view(B, h, w, Cn) if need_feat else None
            Km = Kn if ft else Kb
            rows = dX[R:].float()
            dS_rows = rows[:Km] - rows[Km:]
            if ft:
                dS = torch.cat([dS[:Kb], dS[Kb:] + dS_rows], 0)
            else:
                dS = dS + dS_rows
        if ft:
            Xb, h1b, h2b = sv[8:11]
            need_w_b = ni[4]
            if need_w_b or need_sb:
                dzb = torch.cat([da[:Kb], db[:Kb]]).contiguous()
                dXb, bw1, bw2, bw3 = _mlp_bwd(Xb, h1b, h2b, model.classifier, dzb, need_w_b, need_sb)
                gb = (bw1, bw2, bw3)
                if need_sb:
                    rb = dXb.float()
                    dS = torch.cat([dS[:Kb] + rb[:Kb] - rb[Kb:], dS[Kb:]], 0)
            dSb = dS[:Kb].contiguous() if (need_sb and dS is not None) else None
            dSn = dS[Kb:].contiguous() if (need_sn and dS is not None) else None
            return (dfeat, dSb, dSn, None, *gb, dw1, dw2, dw3)
        return (dfeat, dS if need_sb else None, None, None, dw1, dw2, dw3)


def cls_params(cls):
    return [cls[0].weight, cls[2].weight, cls[4].weight]


class ProtoFn(torch.autograd.Function):
    """F.normalize of the prototype embeddings (pspnet_pop.py:96-99), their similarity matrix (:185-186 / :236-239) and the orthogonality term
    (criterion.py:37-43) as ONE kernel forward and ONE backward (torch: ~50 launches of 5 us).  forward(Ea [Ka,C], Eb [Kb,C] | None) ->
    (Sa, Sb | empty, orth []): rows of the similarity are the `a` prototypes, columns [a ; b]."""

    @staticmethod
    def forward(ctx, Ea, Eb):
        Ea = Ea.detach().float().contiguous()
        Ebc = None if Eb is None else Eb.detach().float().contiguous()
        Sa, Sb, inv, G, orth = ops.pop_proto_fwd(Ea, Ebc)
        ctx.has_b = Eb is not None
        ctx.save_for_backward(Sa, inv, G, *([Sb] if ctx.has_b else []))
        Sb_out = Sb if ctx.has_b else Sa.new_empty(0)
        if not (ctx.has_b and ctx.needs_input_grad[1]):
            # every output of a Function requires grad as soon as ONE input does: without this the frozen base prototypes of ft mode (base_emb.requires_grad False,
            # ft_pop.py:197-203) look trainable to PopHeadFn -- its frozen-base-chain cache never engaged and it ran the base MLP backward for a gradient nobody takes
            ctx.mark_non_differentiable(Sb_out)
        return Sa, Sb_out, orth.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, dSa, dSb, dorth):
        sv = ctx.saved_tensors
        Sa, inv, G = sv[:3]
        Sb = sv[3] if ctx.has_b else None
        need_a, need_b = ctx.needs_input_grad[0], ctx.has_b and ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return None, None
        dSa = None if dSa is None else dSa.float().contiguous()
        dSb = None if (dSb is None or not ctx.has_b) else dSb.float().contiguous()
        dorth = None if dorth is None else dorth.float().reshape(1).contiguous()
        dEa, dEb = ops.pop_proto_bwd(Sa, Sb, inv, G, dSa, dSb, dorth, need_a, need_b)
        return dEa, dEb


# ------------------------------------------------------------------------------------------------ loss
class UpsampleCEFn(torch.autograd.Function):
    """F.interpolate(align_corners=True) + CrossEntropyLoss(ignore_index, mean) of loss/criterion.py:51-52, fused.  `weight` (float32 [K] on the device, no gradient)
    and `label_smoothing` are CrossEntropyLoss's own (loss/criterion.py:33); with the defaults the plain kernels run."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, weight=None, label_smoothing=0.0):
        logits = logits.contiguous()
        out = ops.upsample_ce_fwd(logits, target, ignore_index, weight, label_smoothing)
        ctx.ignore = ignore_index
        ctx.eps = label_smoothing
        ctx.save_for_backward(logits, target, out, weight)
        return out[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logits, target, out, weight = ctx.saved_tensors
        gs = g.detach().reshape(1).float().contiguous()
        return ops.upsample_ce_bwd(logits, target, out, gs, ctx.ignore, weight, ctx.eps), None, None, None, None


class UpsampleCEDiceFn(torch.autograd.Function):
    """(cross-entropy, multiclass soft Dice loss) of the upsampled logits from one pass over the pixels: the hybrid criterion the reference keeps commented out at
    loss/criterion.py:34 (softmax Dice, sum over classes, mean over samples, `smooth` in numerator and denominator; ignored pixels enter neither term).  Two scalars, so
    the caller weighs them; the backward is one launch that takes both upstream gradients from a device buffer."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, weight=None, label_smoothing=0.0, smooth=1.0):
        logits = logits.contiguous()
        out, coef = ops.upsample_ce_dice_fwd(logits, target, ignore_index, weight, label_smoothing, smooth)
        ctx.ignore = ignore_index
        ctx.eps = label_smoothing
        ctx.save_for_backward(logits, target, out, coef, weight)
        return out[0].clone(), out[2].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ce, g_dice):
        logits, target, out, coef, weight = ctx.saved_tensors
        gs = torch.stack([g_ce.detach().reshape(()).float(), g_dice.detach().reshape(()).float()])
        return ops.upsample_ce_dice_bwd(logits, target, out, coef, gs, ctx.ignore, weight, ctx.eps), None, None, None, None, None


class UpsampleFocalFn(torch.autograd.Function):
    """UpsampleCEFn with every pixel's cross-entropy numerator scaled by (1 - p_t)^gamma (focal loss, Lin et al.; include/segland_hip.h has the definition), fused in
    the same kernels: gamma is a plain float, finite and >= 1; `weight` is the focal alpha, the mean divides by the cross-entropy's weight sum."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, gamma, weight=None, label_smoothing=0.0):
        logits = logits.contiguous()
        out = ops.upsample_focal_fwd(logits, target, ignore_index, gamma, weight, label_smoothing)
        ctx.ignore = ignore_index
        ctx.gamma = gamma
        ctx.eps = label_smoothing
        ctx.save_for_backward(logits, target, out, weight)
        return out[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logits, target, out, weight = ctx.saved_tensors
        gs = g.detach().reshape(1).float().contiguous()
        return ops.upsample_focal_bwd(logits, target, out, gs, ctx.ignore, ctx.gamma, weight, ctx.eps), None, None, None, None, None


class UpsampleFocalDiceFn(torch.autograd.Function):
    """UpsampleCEDiceFn with the cross-entropy part focal-modulated (UpsampleFocalFn); the Dice term is the hybrid criterion's, bit for bit."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, gamma, weight=None, label_smoothing=0.0, smooth=1.0):
        logits = logits.contiguous()
        out, coef = ops.upsample_focal_dice_fwd(logits, target, ignore_index, gamma, weight, label_smoothing, smooth)
        ctx.ignore = ignore_index
        ctx.gamma = gamma
        ctx.eps = label_smoothing
        ctx.save_for_backward(logits, target, out, coef, weight)
        return out[0].clone(), out[2].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ce, g_dice):
        logits, target, out, coef, weight = ctx.saved_tensors
        gs = torch.stack([g_ce.detach().reshape(()).float(), g_dice.detach().reshape(()).float()])
        return ops.upsample_focal_dice_bwd(logits, target, out, coef, gs, ctx.ignore, ctx.gamma, weight, ctx.eps), None, None, None, None, None, None


class UpsampleLovaszFn(torch.autograd.Function):
    """(cross-entropy, multiclass soft Dice loss or None, Lovasz-softmax loss) of the upsampled logits.  The cross-entropy (plain, weighted / smoothed, focal for
    gamma >= 1) and, with `dice`, the Dice term come from the forward of UpsampleCEFn / UpsampleFocalFn / UpsampleCEDiceFn / UpsampleFocalDiceFn, bit for bit; the
    Lovasz term (include/segland_hip.h has the definition: binned errors, no sort; classes = "present", batch-wide, no class weights) adds a histogram pass and a scan.
    The backward is ONE launch that takes the three upstream gradients from a device buffer."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, gamma=0.0, weight=None, label_smoothing=0.0, dice=False, smooth=1.0):
        logits = logits.contiguous()
        coef = None
        if dice:
            if gamma > 0.0:
                out, coef = ops.upsample_focal_dice_fwd(logits, target, ignore_index, gamma, weight, label_smoothing, smooth)
            else:
                out, coef = ops.upsample_ce_dice_fwd(logits, target, ignore_index, weight, label_smoothing, smooth)
        elif gamma > 0.0:
            out = ops.upsample_focal_fwd(logits, target, ignore_index, gamma, weight, label_smoothing)
        else:
            out = ops.upsample_ce_fwd(logits, target, ignore_index, weight, label_smoothing)
        lov, table = ops.upsample_lovasz_fwd(logits, target, ignore_index)
        ctx.ignore = ignore_index
        ctx.gamma = gamma
        ctx.eps = label_smoothing
        ctx.dice = dice
        ctx.save_for_backward(logits, target, out, coef, table, weight)
        if dice:
            return out[0].clone(), out[2].clone(), lov[0].clone()
        return out[0].clone(), None, lov[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ce, g_dice, g_lov):
        logits, target, out, coef, table, weight = ctx.saved_tensors
        zero = g_ce.new_zeros(())
        gs = torch.stack([(zero if g is None else g).detach().reshape(()).float() for g in (g_ce, g_dice if ctx.dice else None, g_lov)])
        return ops.upsample_lovasz_bwd(logits, target, out, coef, table, gs, ctx.ignore, ctx.gamma, weight, ctx.eps), None, None, None, None, None, None, None
