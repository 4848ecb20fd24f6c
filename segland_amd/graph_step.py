"""The training step as HIP graphs: forward, loss, backward, gradient-norm clip and both AdamW steps of the loop body (train_base.py:250-264)
are captured once per input shape and replayed, so a step costs one graph launch instead of ~750 (PSPNet-POP) / ~1300 (Swin-POP) kernel
launches issued from Python.  At 16 tiles per GPU the ResNet step is GPU-bound either way; at the 8 tiles per GPU of the Swin configuration
(BASELINE config 5) and in fine-tuning the launches were the bottleneck.

What makes the step replayable: every kernel of the path takes its stream from torch (ops._s), nothing on the path synchronises or reads
a value back, BatchNorm's `num_batches_tracked` and running statistics are updated by kernels, DropPath / Dropout2d draw from torch's
graph-safe Philox state, and segland_amd.optim.AdamW keeps its step-dependent scalars (bias corrections, the groups' lr and weight
decay) in device memory that `graph_prepare()` refreshes before each replay.  Not captured: DistributedDataParallel (its reducer and
RCCL work run eagerly) -- `eligible()` says no and the caller keeps `train_iteration`.

ONE lifecycle (`StepLifecycle`) serves both step graphs -- `GraphedStep` here (one graph: one GPU, fine-tuning, the benchmark) and
`bucket_step.GraphedBucketStep` (two or three graphs around the gradient all-reduces of a BucketedReplica): the signature key, the warm-up
per signature, the attempt policy, the capture preamble, what a capture commits, and the replay path with its cache invalidation.  A class
says how it differs through five hooks: `_eager`, `_capture_graphs` (record), `_agree` (is the outcome of an attempt local or the ranks'),
`_warn_failed` (its log line) and `_replay`."""
import logging
import os

import torch

from . import functional, ops


STATS = {'captures': 0, 'replays': 0, 'failures': 0}          # process-wide counters (tests / logs: did the drivers really replay?)


def eligible(model, optimizer, device, need_adamw=True):
    from .optim import AdamW
    return (os.environ.get('SEGLAND_STEP_GRAPH', '1') != '0' and torch.cuda.is_available() and torch.device(device).type == 'cuda'
            and (isinstance(optimizer, AdamW) or not need_adamw) and not isinstance(model, torch.nn.parallel.DistributedDataParallel))


def _detached(out):
    """Losses handed to the caller without their autograd graph: a loss the caller keeps would keep this step's graph -- and its
    AccumulateGrad nodes, bound to THIS stream -- alive into a capture on another stream (autograd then synchronises the two streams,
    which a capture cannot contain)."""
    if isinstance(out, dict):
        return {k: _detached(v) for k, v in out.items()}
    if isinstance(out, (tuple, list)):
        return type(out)(_detached(v) for v in out)
    return out.detach() if torch.is_tensor(out) else out


class StepLifecycle:
    """A step of `model` captured once per input signature and replayed.  The first `warmup` calls per signature run eagerly (lazy allocations,
    optimizer state, weight-preparation tables); the next one is an ATTEMPT: the step is recorded into `graph` without running, and when the
    attempt stands (`_agree`) this very call is the first replay.  A failed attempt issues this step eagerly, once; the next call attempts
    again without a new warm-up; after the third failure the object stays eager.  One signature is current at a time.  The returned tensors
    are the graphs' static outputs: read them (`.item()`, `float()`) before the next call.  `optimizer`: a segland_amd.optim optimizer whose
    step() is inside the recorded step (its step counts and hyper-parameters are advanced / uploaded before every replay) or None.

    The hooks of a subclass:
      _eager(*tensors)            the step issued kernel by kernel -> its detached results
      _capture_graphs(*tensors)   -> (graph(s), outputs): the step recorded on `tensors` (self.static_in); nothing executes
      _agree(ok, key)             does the attempt stand?  ok: recording went through here (default: the local outcome)
      _warn_failed(err, last)     the log line of a failed attempt; err: what recording raised HERE or None, last: the object stays eager from now on
      _replay(tensors)            launch the graph(s)"""
    eager_reason = None                                     # not None: why every step is issued kernel by kernel (no key work, no attempt)

    def __init__(self, model, optimizer, warmup):
        self.model, self.optimizer, self.warmup = model, optimizer, warmup
        self.inner = functional.unwrapped(model)            # the drivers hand over what engine.data_parallel returned: key, `baked` and gradients are the module's behind it
        self.seen, self.key, self.graph = {}, None, None
        self.static_in, self.static_out, self.static_grads = None, None, None
        self.replays, self.failures, self.baked = 0, 0, None
        self.bn_training = True

    def _agree(self, ok, key):
        return ok

    def _state_key(self, tensors):
        # ft mode: the frozen base classifier's prototype rows are cached tensors baked into a captured step (functional._base_chain): what they are computed from is
        # part of the key, so a weight change behind the graph (load_state_dict, init_cls_n) re-captures instead of replaying stale rows
        m = self.inner
        return tuple((tuple(t.shape), t.dtype) for t in tensors) + (sum(1 for p in m.parameters() if p.requires_grad), sum(1 for x in m.modules() if x.training),
                                                                    functional.base_chain_key(m))

    def _attempt(self, tensors, key):
        """One capture attempt.  True: self.graph holds this step on self.static_in, not yet run."""
        self.graph, self.key, err = None, None, None        # drop the older graph(s) (and their pool) first
        try:
            self.static_in = tuple(t.clone() for t in tensors)
            if self.optimizer is not None:
                self.optimizer.capture_begin()
            functional.flush_num_batches_tracked()
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            graph, out = self._capture_graphs(*self.static_in)
        except Exception as e:                              # noqa: BLE001  something on the path still needed the host (a lazy upload, a read-back)
            err = e
            if torch.cuda.is_available():
                ops.after_failed_capture()
        if not self._agree(err is None, key):
            functional.after_failed_capture()               # counters queued and caches filled by the attempt (here or on the rank that did capture): nothing of it ran
            self.failures += 1
            STATS['failures'] += 1
            last = self.failures >= 3
            self._warn_failed(err, last)
            if last:
                self.warmup = float('inf')
            return False
        m = self.inner
        self.graph, self.static_out, self.key = graph, out, key
        self.baked = m.__dict__.get('_sl_base_chain')       # tensors of the cache entry the captured launches read: alive as long as the graphs are
        self.bn_training = any(isinstance(x, torch.nn.modules.batchnorm._BatchNorm) and x.training for x in m.modules())
        # the gradients the replays write: tensors of the graphs' pool that the parameters keep pointing at
        self.static_grads = [(p, p.grad) for p in m.parameters() if p.grad is not None]
        STATS['captures'] += 1
        return True

    def __call__(self, *tensors):
        if self.eager_reason is not None:
            return self._eager(*tensors)
        key = self._state_key(tensors)
        if key != self.key or self.graph is None:
            n = self.seen.get(key, 0)
            if n < self.warmup:
                self.seen[key] = n + 1
                return self._eager(*tensors)
            if not self._attempt(tensors, key):
                return self._eager(*tensors)                # nothing of the failed attempt has run: this is the step's one and only execution
        else:                                               # (the step that captured holds its batch in static_in already)
            for dst, src in zip(self.static_in, tensors):
                dst.copy_(src, non_blocking=True)
        for p, g in self.static_grads:                      # an eager step in between (odd last batch) or zero_grad() re-pointed .grad
            if p.grad is not g:
                p.grad = g
        self._replay(tensors)
        self.replays += 1
        STATS['replays'] += 1
        # A replay runs no Python: the optimizer kernel, the BN running-statistics kernels and the weight re-preparation (which sits BEFORE the
        # optimizer in the captured order, so the prepared copies lag the parameters by one step) all went through raw pointers.  Invalidate every
        # host-side cache keyed on them (prepared weights, BN eval coefficients, the captured eval feature graph): the next eager forward --
        # validation between epochs -- must see this replay's weights and statistics.
        if self.optimizer is not None:
            functional.weights_changed()
        if self.bn_training:
            functional.running_stats_changed()
        return self.static_out


class GraphedStep(StepLifecycle):
    """`body(*tensors)` -- a function of GPU tensors that launches the kernels of a step and returns tensors -- as ONE graph; the outcome of an
    attempt is this process's own."""

    def __init__(self, body, model, optimizer=None, warmup=3):
        super().__init__(model, optimizer, warmup)
        self.body = body

    def _eager(self, *tensors):
        return _detached(self.body(*tensors))

    def _capture_graphs(self, *tensors):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode='thread_local'):
            out = self._eager(*tensors)
        return g, out

    def _warn_failed(self, err, last):
        logging.getLogger('Segmentation').warning('graph_step: capture failed (%s: %s); %s', type(err).__name__, str(err).splitlines()[0] if str(err) else '',
                                                  'staying eager' if last else 'one more eager step, then another attempt')

    def _replay(self, tensors):
        if self.optimizer is not None:
            self.optimizer.graph_prepare()
        self.graph.replay()


class GraphedTrainStep(GraphedStep):
    """Callable with the signature and results of train_base.train_iteration(model, optimizer, loss_scaler, img, mask): the whole loop body
    (train_base.py:250-264) including clip + both AdamW steps in the graph."""

    def __init__(self, step_fn, model, optimizer, loss_scaler, double_step=True, warmup=3):
        super().__init__(lambda img, mask: step_fn(model, optimizer, loss_scaler, img, mask, double_step=double_step), model, optimizer, warmup)
