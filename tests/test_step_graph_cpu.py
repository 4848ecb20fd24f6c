"""The capture-and-replay lifecycle of the step graphs (segland_amd/graph_step.py: StepLifecycle) on the CPU: recorded stand-ins take the place of HIP graphs
(recording does not run the step, replay() does), so key, warm-up, attempt policy, static inputs and counters are exercised without a GPU.  The bucket step's use
of the same lifecycle over two gloo ranks: test_drivers_cpu.py."""
import logging

import torch

from test_drivers_cpu import _ToyOpt


class _Recorded:
    def __init__(self, fn, args, slot):
        self.fn, self.args, self.slot = fn, args, slot

    def replay(self):
        self.slot.update({k: v.detach() for k, v in self.fn(*self.args).items()})


def _toy():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4))


def _body(m, opt):
    def body(x, y):
        opt.zero_grad(set_to_none=True)
        loss = ((m(x) - y) ** 2).mean()
        loss.backward()
        opt.step()
        return {'total_loss': loss}
    return body


def _make_step(m, opt, warmup, fail=0):
    from segland_amd import graph_step

    class Step(graph_step.GraphedStep):
        attempts = 0

        def _capture_graphs(self, *tensors):
            self.attempts += 1
            assert len(tensors) == len(self.static_in) and all(a is b for a, b in zip(tensors, self.static_in))
            if self.attempts <= fail:
                raise RuntimeError('injected: recording fails on attempt %d' % self.attempts)
            slot = {}
            return _Recorded(self.body, tensors, slot), slot
    return Step(_body(m, opt), m, opt, warmup=warmup)


def _data(shapes):
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(b, 8, generator=g), torch.randn(b, 4, generator=g)) for b in shapes]


def _eager_states(data):
    m = _toy()
    body = _body(m, _ToyOpt(m.parameters(), lr=0.05))
    out = []
    for x, y in data:
        loss = float(body(x, y)['total_loss'].detach())
        out.append((loss, [p.detach().clone() for p in m.parameters()]))
    return out


def _same(m, loss, want):
    return float(loss['total_loss']) == want[0] and all(torch.equal(p, w) for p, w in zip(m.parameters(), want[1]))


def test_graphed_step_lifecycle_warmup_capture_replay_and_signatures():
    """warmup=2, eight steps, batch sizes 5 5 5 5 3 3 3 5: two warm-up steps and a capture per NEW signature (the capturing step is the first replay), a re-capture
    without warm-up on the return to the first one (one key is current at a time); parameters and losses equal the eager loop's bit for bit after every step."""
    from segland_amd import graph_step
    data = _data([5, 5, 5, 5, 3, 3, 3, 5])
    want = _eager_states(data)
    m = _toy()
    step = _make_step(m, _ToyOpt(m.parameters(), lr=0.05), warmup=2)
    before = dict(graph_step.STATS)
    trace = []
    for k, (x, y) in enumerate(data):
        assert _same(m, step(x, y), want[k]), 'step %d differs from the eager loop' % k
        trace.append((step.attempts, step.replays, step.graph is not None))
    assert trace == [(0, 0, False), (0, 0, False), (1, 1, True), (1, 2, True),
                     (1, 2, True), (1, 2, True), (2, 3, True),          # the other shape: eager beside the older graph twice, then its own capture
                     (3, 4, True)]
    assert step.failures == 0 and step.key == step._state_key(data[-1])
    assert {k: graph_step.STATS[k] - before[k] for k in before} == {'captures': 3, 'replays': 4, 'failures': 0}


def test_graphed_step_failed_attempts_run_eagerly_then_recover(caplog):
    """Recording raises on the first two attempts: those steps run eagerly, once, the next call attempts again without a new warm-up, the third attempt captures."""
    from segland_amd import graph_step
    data = _data([5] * 7)
    want = _eager_states(data)
    m = _toy()
    step = _make_step(m, _ToyOpt(m.parameters(), lr=0.05), warmup=2, fail=2)
    before = dict(graph_step.STATS)
    trace = []
    with caplog.at_level(logging.WARNING, logger='Segmentation'):
        for k, (x, y) in enumerate(data):
            assert _same(m, step(x, y), want[k]), 'step %d differs from the eager loop' % k
            trace.append((step.attempts, step.failures, step.replays, step.graph is not None))
    assert trace == [(0, 0, 0, False), (0, 0, 0, False), (1, 1, 0, False), (2, 2, 0, False), (3, 2, 1, True), (3, 2, 2, True), (3, 2, 3, True)]
    assert {k: graph_step.STATS[k] - before[k] for k in before} == {'captures': 1, 'replays': 3, 'failures': 2}
    said = [r.getMessage() for r in caplog.records if r.getMessage().startswith('graph_step: capture failed')]
    assert len(said) == 2 and all(s.endswith('one more eager step, then another attempt') and 'RuntimeError: injected' in s for s in said), said


def test_graphed_step_stays_eager_after_three_failed_attempts(caplog):
    from segland_amd import graph_step
    data = _data([5] * 8)
    want = _eager_states(data)
    m = _toy()
    step = _make_step(m, _ToyOpt(m.parameters(), lr=0.05), warmup=2, fail=1 << 30)
    before = dict(graph_step.STATS)
    with caplog.at_level(logging.WARNING, logger='Segmentation'):
        for k, (x, y) in enumerate(data):
            assert _same(m, step(x, y), want[k]), 'step %d differs from the eager loop' % k
    assert (step.attempts, step.failures, step.replays, step.graph, step.key) == (3, 3, 0, None, None) and step.warmup == float('inf')
    assert {k: graph_step.STATS[k] - before[k] for k in before} == {'captures': 0, 'replays': 0, 'failures': 3}
    said = [r.getMessage() for r in caplog.records if r.getMessage().startswith('graph_step: capture failed')]
    assert [s.rsplit('; ', 1)[1] for s in said] == ['one more eager step, then another attempt'] * 2 + ['staying eager'], said


class _FtStub(torch.nn.Module):
    """What functional.base_chain_key looks at: `is_ft`, a frozen `base_emb` and a five-layer `classifier` (weights at 0, 2, 4)."""
    is_ft = True

    def __init__(self, frozen=True):
        super().__init__()
        torch.manual_seed(1)
        self.base_emb = torch.nn.Parameter(torch.randn(7, 16), requires_grad=False)
        self.classifier = torch.nn.Sequential(torch.nn.Conv2d(16, 16, 1, bias=False), torch.nn.ReLU(), torch.nn.Conv2d(16, 8, 1, bias=False), torch.nn.ReLU(),
                                              torch.nn.Conv2d(8, 1, 1, bias=False))
        self.classifier_n = torch.nn.Conv2d(16, 1, 1)
        self.classifier.requires_grad_(not frozen)


class _Holder:
    def __init__(self, module):
        self.module = module


def test_base_chain_key_and_step_key_behind_wrappers():
    """The fine-tune driver hands the step graph engine.data_parallel(model) -- a ModuleWrapper on one GPU: the base-chain part of the key must engage behind it (and
    behind a replica / DDP-style `.module.module`), or a change of the frozen base classifier replays stale prototype rows."""
    from segland_amd import engine, graph_step
    from segland_amd import functional as sf
    m = _FtStub()
    k = sf.base_chain_key(m)
    assert isinstance(k, tuple)
    assert sf.base_chain_key(engine.ModuleWrapper(m)) == k and sf.base_chain_key(_Holder(_Holder(m))) == k
    assert sf.unwrapped(_Holder(engine.ModuleWrapper(m))) is m and sf.unwrapped(m) is m
    x = torch.zeros(2, 3)
    for wrap in (lambda v: v, engine.ModuleWrapper):
        gs = graph_step.GraphedStep(lambda *a: None, wrap(m))
        k0 = gs._state_key((x,))
        assert k0 == gs._state_key((x,)) and k0[-1] == sf.base_chain_key(m)
        with torch.no_grad():
            m.classifier[0].weight.add_(0.0)              # an in-place write (what load_state_dict does): the version counter moves
        assert gs._state_key((x,)) != k0
    t = _FtStub(frozen=False)
    assert sf.base_chain_key(t) is None and sf.base_chain_key(engine.ModuleWrapper(t)) is None
    assert graph_step.GraphedStep(lambda *a: None, engine.ModuleWrapper(t))._state_key((x,))[-1] is None
