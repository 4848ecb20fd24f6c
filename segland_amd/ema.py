"""Exponential moving average of a model's weights, updated by ONE kernel launch per optimizer step (csrc/optim.hip sl_ema_multi) that sits behind the optimizer
kernel -- also inside a captured training step, where a replay runs no Python: attach it to the optimizer (segland_amd.optim.AdamW / SGD .attach_ema) and every step
path updates the shadows.  Validation and checkpoints of the averaged weights go through `applied()` / `model_state_dict()`.

    ema = ModelEma(model, decay=0.999)          # after the model is on its device and in the mode it trains in
    optimizer.attach_ema(ema)
    ... train ...
    with ema.applied():                         # the averaged weights stand in the model, every cache derived from weights / running statistics follows
        validate(model, ...)
    torch.save(ema.model_state_dict(), path)    # the model's state_dict with the averaged tensors in it
"""
import contextlib
import struct

import numpy as np
import torch

from . import functional, ops


class ModelEma:
    """Tracked, fixed at construction: every parameter with requires_grad and the running_mean / running_var of every BatchNorm module in training mode at that moment
    (a frozen backbone costs nothing); everything else is read from the live model whenever the averaged weights are applied or saved.  Names are the keys of
    model.state_dict() of the model as given (a wrapped model keeps its `module.` prefix).  Shadows are fp32 clones that are never reallocated, so a captured launch
    stays valid across load_state_dict() and applied().

    decay_at(t) = min(decay, (1 + t) / (10 + t)) with warm-up, decay without; t = updates done so far; the kernel reads w = float32(1 - decay_at(t)) from device memory.
    Data-parallel runs: every rank holds the same weights, hence the same shadows; nothing is communicated."""

    def __init__(self, model, decay, warmup=True):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError('ModelEma: decay must lie in (0, 1) (got %r)' % (decay,))
        self.model, self.decay, self.warmup, self.updates = model, decay, bool(warmup), 0
        live = model.state_dict(keep_vars=True)             # the Parameter / buffer objects themselves
        tracked = {id(p) for p in model.parameters() if p.requires_grad}
        for mod in model.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm) and mod.training and mod.running_mean is not None:
                tracked.update((id(mod.running_mean), id(mod.running_var)))
        self.names, self._alias, first = [], {}, {}
        for key, t in live.items():
            if id(t) in tracked:
                if id(t) not in first:                      # a tensor under two keys (tied weights) has one shadow
                    first[id(t)] = key
                    self.names.append(key)
                self._alias[key] = first[id(t)]
        self._live = [live[k] for k in self.names]
        for k, t in zip(self.names, self._live):
            if t.dtype != torch.float32:                    # the exchange of applied() is exact only between equal formats; the project keeps master weights in fp32
                raise TypeError('ModelEma: %s is %s; tracked tensors must be float32' % (k, t.dtype))
        self.shadows = {k: t.detach().clone(memory_format=torch.contiguous_format) for k, t in zip(self.names, self._live)}
        self._captured = False
        self._table = self._w = None
        if self.names and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in self._live):
            rec, chunks = bytearray(), 0
            for k, t in zip(self.names, self._live):
                rec += struct.pack('<QQqq', self.shadows[k].data_ptr(), t.data_ptr(), t.numel(), chunks)
                chunks += (t.numel() + 4095) // 4096
            dev = self._live[0].device
            self._table = torch.frombuffer(rec, dtype=torch.uint8).to(dev)
            self._chunks, self._ptrs = chunks, [t.data_ptr() for t in self._live]
            self._w = torch.zeros(1, dtype=torch.float32, device=dev)

    # ---- decay schedule
    def decay_at(self, t):
        return min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay

    def weight_at(self, t):
        """w of update number t (0-based): 1 - decay_at(t) in double, rounded once to float32 -- the value the kernel multiplies by."""
        return float(np.float32(1.0 - self.decay_at(t)))

    # ---- the update, called by the optimizer at the end of step()
    @torch.no_grad()
    def update(self):
        if not self.names:
            return
        if self._table is None:                             # not contiguous fp32 GPU tensors: the same formula with torch ops (host logic on the CPU; no hot path)
            w = self.weight_at(self.updates)
            for k, t in zip(self.names, self._live):
                self.shadows[k].add_((t.detach() - self.shadows[k]).mul_(w))
            self.updates += 1
            return
        if torch.cuda.is_current_stream_capturing():        # a captured step does not execute: graph_prepare() stores each replay's w and counts it
            ops.ema_multi(self._table, len(self.names), self._chunks, self._w)
            self._captured = True
            return
        for k, t, ptr in zip(self.names, self._live, self._ptrs):
            if t.data_ptr() != ptr:
                raise RuntimeError('ModelEma: %s was reallocated after construction (model.to() / a replaced .data?): build the ModelEma after the model is in place' % k)
        ops.store_floats(self._w, [self.weight_at(self.updates)])      # kernel arguments of a one-block launch: no host -> device copy
        ops.ema_multi(self._table, len(self.names), self._chunks, self._w)
        self.updates += 1

    # ---- whole-step HIP graphs: the protocol of optim.SGD, driven by the optimizer this is attached to
    def capture_begin(self):
        self._captured = False

    def graph_prepare(self):
        if self._captured:
            ops.store_floats(self._w, [self.weight_at(self.updates)])
            self.updates += 1

    # ---- the averaged weights in the model
    @torch.no_grad()
    def _exchange(self):
        if self.names:
            live = [t.detach() for t in self._live]
            shadows = [self.shadows[k] for k in self.names]
            tmp = [t.clone() for t in live]
            torch._foreach_copy_(live, shadows)
            torch._foreach_copy_(shadows, tmp)
        # prepared GEMM copies, BN eval coefficients and the eval feature graph are keyed on these two
        functional.weights_changed()
        functional.running_stats_changed()

    @contextlib.contextmanager
    def applied(self):
        """Inside: the model holds the averaged tensors and the shadows hold the raw ones, exchanged IN PLACE (every pointer a captured step has baked in stays
        valid); on exit they are exchanged back.  Do not step the optimizer inside."""
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()

    def model_state_dict(self):
        """The model's state_dict (same keys, the on-disk format of drivers.save_checkpoint) with every tracked entry replaced by its shadow."""
        out = self.model.state_dict()
        for key, name in self._alias.items():
            out[key] = self.shadows[name]
        return out

    # ---- checkpoints
    def state_dict(self):
        return {'decay': self.decay, 'warmup': self.warmup, 'updates': self.updates, 'shadows': dict(self.shadows)}

    @torch.no_grad()
    def load_state_dict(self, state):
        """Copies IN PLACE (a captured graph keeps reading the same shadow tensors); a missing or unexpected name is an error that names it."""
        got = state['shadows']
        missing, unexpected = [k for k in self.names if k not in got], [k for k in got if k not in self.shadows]
        if missing or unexpected:
            raise KeyError('ModelEma.load_state_dict: missing %s, unexpected %s' % (missing or 'none', unexpected or 'none'))
        for k in self.names:
            if tuple(got[k].shape) != tuple(self.shadows[k].shape):
                raise ValueError('ModelEma.load_state_dict: %s has shape %s, the model has %s' % (k, tuple(got[k].shape), tuple(self.shadows[k].shape)))
        for k in self.names:
            self.shadows[k].copy_(got[k])
        self.decay, self.warmup, self.updates = float(state['decay']), bool(state['warmup']), int(state['updates'])

    @torch.no_grad()
    def reset_to_model(self):
        """Shadows := the live tensors, updates := 0 (a resume from a state file written without EMA)."""
        for k, t in zip(self.names, self._live):
            self.shadows[k].copy_(t.detach())
        self.updates = 0
