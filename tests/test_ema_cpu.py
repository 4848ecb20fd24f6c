"""Weight EMA (--ema-decay), CPU side: sl_ema_multi exists, is declared with five arguments and validates before any launch while its neighbours keep their
signatures; the decay schedule; both drivers' parsers carry --ema-decay / --ema-warmup, bad values and torch's optimizers are refused with a ValueError; and the host
logic of segland_amd.ema.ModelEma on a tiny CPU model (torch-op fallback of update()): tracked set, float64 recurrence, state_dict round trip in place, applied(),
model_state_dict() and the 'ema' entry of the training state.  The kernel, the optimizer hook, the captured step and the drivers: test_ema_gpu.py."""
import ctypes as C
import logging
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    from segland_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_ema_entry_is_exported_and_declared_and_the_neighbours_keep_their_signatures(lib):
    from segland_amd import _lib, ops
    decl = _lib.declared_functions()
    assert hasattr(lib, 'sl_ema_multi') and 'sl_ema_multi' in decl
    restype, args = decl['sl_ema_multi']
    assert restype is C.c_int and args == [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    assert [len(decl[n][1]) for n in ('sl_adamw_multi', 'sl_adamw_multi_dev', 'sl_sgd_multi', 'sl_store_floats')] == [13, 10, 7, 4]
    assert callable(ops.ema_multi)


def test_ema_entry_validates_before_any_launch(lib):
    """SL_EINVAL (-1) with a message and no launch (the pointers are not device memory: a launch would fault) for every null, n = 0 and total_chunks = 0"""
    d = C.c_void_p(16)
    err = lambda: lib.sl_last_error_string().decode()
    assert lib.sl_ema_multi(None, 1, 1, d, None) == -1 and 'ema_multi' in err() and 'null' in err()
    assert lib.sl_ema_multi(d, 1, 1, None, None) == -1 and 'ema_multi' in err() and 'null' in err()
    assert lib.sl_ema_multi(None, 1, 1, None, None) == -1 and 'null' in err()
    assert lib.sl_ema_multi(d, 0, 1, d, None) == -1 and 'ema_multi' in err() and 'positive' in err()
    assert lib.sl_ema_multi(d, -3, 1, d, None) == -1 and 'positive' in err()
    assert lib.sl_ema_multi(d, 1, 0, d, None) == -1 and 'ema_multi' in err() and 'positive' in err()
    assert lib.sl_ema_multi(d, 1, -1, d, None) == -1 and 'positive' in err()


def test_ema_op_refuses_cpu_tensors(lib):
    from segland_amd import ops
    with pytest.raises(RuntimeError, match='not on the GPU'):
        ops.ema_multi(torch.zeros(32, dtype=torch.uint8), 1, 1, torch.zeros(1))


# --------------------------------------------------------------------------------------------- schedule
def _lin():
    return torch.nn.Linear(2, 2)


def test_decay_schedule():
    from segland_amd.ema import ModelEma
    e = ModelEma(_lin(), 0.999)
    assert e.decay_at(0) == 0.1 and e.decay_at(90) == 0.91
    assert e.decay_at(10 ** 6) == 0.999 and e.decay_at(8990) == 0.999 and e.decay_at(8989) < 0.999
    assert all(e.decay_at(t) <= e.decay_at(t + 1) <= 0.999 for t in range(0, 20000, 7))
    assert e.weight_at(0) == float(np.float32(0.9)) and e.weight_at(10 ** 6) == float(np.float32(1.0 - 0.999))
    flat = ModelEma(_lin(), 0.9, warmup=False)
    assert [flat.decay_at(t) for t in (0, 1, 90, 10 ** 6)] == [0.9] * 4
    low = ModelEma(_lin(), 0.05)                      # a decay below the warm-up's first value caps from the start
    assert low.decay_at(0) == 0.05 and low.decay_at(100) == 0.05
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='decay'):
            ModelEma(_lin(), bad)


# --------------------------------------------------------------------------------------------- parsers and refusals
@pytest.mark.parametrize('ft', [False, True])
def test_parsers_carry_the_two_flags(ft):
    from segland_amd.drivers import build_parser
    p = build_parser(ft)
    a = p.parse_args([])
    assert a.ema_decay == 0.0 and a.ema_warmup is True
    a = p.parse_args(['--ema-decay', '0.999', '--ema-warmup', 'false'])
    assert a.ema_decay == 0.999 and a.ema_warmup is False
    assert p.parse_args(['--ema-warmup', 'yes']).ema_warmup is True


@pytest.mark.parametrize('ft', [False, True])
def test_bad_decays_are_refused_with_the_value(ft):
    from segland_amd.drivers import build_parser, ema_decay, make_ema
    assert ema_decay(0) == 0.0 and ema_decay(0.5) == 0.5 and ema_decay('0.9999') == 0.9999
    for bad in ('1.0', '-0.1', 'nan', '1.5', 'inf'):
        a = build_parser(ft).parse_args(['--ema-decay', bad])
        with pytest.raises(ValueError) as ei:
            ema_decay(a.ema_decay)
        assert repr(float(bad)) in str(ei.value), str(ei.value)
        with pytest.raises(ValueError) as ei:
            make_ema(a, _lin(), None)
        assert repr(float(bad)) in str(ei.value)


def test_off_makes_nothing_and_torch_optimizers_are_refused(caplog):
    from segland_amd.drivers import build_parser, make_ema
    from segland_amd.optim import SGD, AdamW
    m = _lin()
    assert make_ema(build_parser(False).parse_args([]), m, torch.optim.AdamW(m.parameters())) is None
    for ft, opt in ((False, torch.optim.AdamW(m.parameters())), (True, torch.optim.SGD(m.parameters(), lr=0.1))):
        with pytest.raises(ValueError) as ei:
            make_ema(build_parser(ft).parse_args(['--ema-decay', '0.99']), m, opt)
        assert 'segland_amd.optim' in str(ei.value) and type(opt).__name__ in str(ei.value) and '0.99' in str(ei.value)
    # the HIP optimizers take it; one log line, only when on and asked for
    for cls in (AdamW, SGD):
        opt = cls(m.parameters(), lr=0.1)
        assert opt._ema is None
        with caplog.at_level(logging.INFO, logger='Segmentation'):
            ema = make_ema(build_parser(False).parse_args(['--ema-decay', '0.99', '--ema-warmup', '0']), m, opt, log=True)
        assert opt._ema is ema and ema.decay == 0.99 and ema.warmup is False
    msgs = [r.getMessage() for r in caplog.records]
    assert len(msgs) == 2 and all(s.startswith('weight EMA: decay 0.99, 2 tensors (6 values)') for s in msgs), msgs


# --------------------------------------------------------------------------------------------- host logic on a tiny CPU model
class Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 3)
        self.bn_train = torch.nn.BatchNorm2d(4)
        self.bn_eval = torch.nn.BatchNorm2d(4)
        self.frozen = torch.nn.Parameter(torch.randn(5), requires_grad=False)


def _tiny():
    from segland_amd.engine import ModuleWrapper
    torch.manual_seed(3)
    m = Tiny()
    with torch.no_grad():
        for bn in (m.bn_train, m.bn_eval):
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
    m.train()
    m.bn_eval.eval()
    return ModuleWrapper(m)


TRACKED = ['module.conv.weight', 'module.conv.bias', 'module.bn_train.weight', 'module.bn_train.bias', 'module.bn_train.running_mean', 'module.bn_train.running_var',
           'module.bn_eval.weight', 'module.bn_eval.bias']


def _perturb(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for t in model.state_dict(keep_vars=True).values():
            if t.dtype.is_floating_point:
                t.add_(torch.randn(t.shape, generator=g) * 0.1)
            else:
                t.add_(1)


def test_tracked_set():
    from segland_amd.ema import ModelEma
    model = _tiny()
    ema = ModelEma(model, 0.9)
    assert ema.names == TRACKED and list(ema.shadows) == TRACKED and ema.updates == 0
    live = model.state_dict(keep_vars=True)
    for k in TRACKED:
        s = ema.shadows[k]
        assert s.dtype == torch.float32 and torch.equal(s, live[k]) and s.data_ptr() != live[k].data_ptr() and not s.requires_grad
    assert set(live) - set(TRACKED) == {'module.frozen', 'module.bn_train.num_batches_tracked', 'module.bn_eval.running_mean', 'module.bn_eval.running_var',
                                        'module.bn_eval.num_batches_tracked'}
    # fixed at construction: a later mode change does not move the set
    model.module.bn_eval.train()
    model.module.bn_train.eval()
    ema.update()
    assert ema.names == TRACKED and ema.updates == 1


@pytest.mark.parametrize('warmup', [True, False])
def test_update_follows_the_float64_recurrence(warmup):
    from segland_amd.ema import ModelEma
    model = _tiny()
    ema = ModelEma(model, 0.9, warmup=warmup)
    live = model.state_dict(keep_vars=True)
    ref = {k: live[k].detach().double().clone() for k in TRACKED}
    T, M = 12, 0.0
    for t in range(T):
        _perturb(model, 100 + t)
        w = float(np.float32(1.0 - (min(0.9, (1.0 + t) / (10.0 + t)) if warmup else 0.9)))
        assert ema.weight_at(t) == w
        for k in TRACKED:
            src = live[k].detach().double()
            M = max(M, float(src.abs().max()), float(ref[k].abs().max()))
            ref[k] += (src - ref[k]) * w
        ema.update()
    assert ema.updates == T
    worst = max(float((ema.shadows[k].double() - ref[k]).abs().max()) for k in TRACKED)
    bound = 4 * T * 2.0 ** -24 * M               # at most three roundings per step on magnitudes <= 2M, earlier error carried with a factor below 1
    print('warmup %s: max |err| %.3g, bound %.3g' % (warmup, worst, bound))
    assert worst <= bound
    assert max(float((ema.shadows[k] - live[k].detach()).abs().max()) for k in TRACKED) > 1e-3         # an average, not a copy


def test_state_dict_round_trip_keeps_tensor_identities_and_updates():
    from segland_amd.ema import ModelEma
    model = _tiny()
    ema = ModelEma(model, 0.99)
    for t in range(3):
        _perturb(model, t)
        ema.update()
    state = ema.state_dict()
    assert set(state) == {'decay', 'warmup', 'updates', 'shadows'} and state['updates'] == 3 and list(state['shadows']) == TRACKED
    saved = {k: v.clone() for k, v in state['shadows'].items()}
    other = ModelEma(_tiny(), 0.5, warmup=False)
    ids = {k: (id(v), v.data_ptr()) for k, v in other.shadows.items()}
    other.load_state_dict({'decay': 0.99, 'warmup': True, 'updates': 3, 'shadows': saved})
    assert (other.decay, other.warmup, other.updates) == (0.99, True, 3)
    for k in TRACKED:
        assert (id(other.shadows[k]), other.shadows[k].data_ptr()) == ids[k] and torch.equal(other.shadows[k], saved[k])
    with pytest.raises(KeyError, match='module.conv.bias'):
        other.load_state_dict({'decay': 0.99, 'warmup': True, 'updates': 3, 'shadows': {k: v for k, v in saved.items() if k != 'module.conv.bias'}})
    with pytest.raises(KeyError, match='module.stranger'):
        other.load_state_dict({'decay': 0.99, 'warmup': True, 'updates': 3, 'shadows': dict(saved, **{'module.stranger': torch.zeros(1)})})
    assert other.updates == 3 and all(torch.equal(other.shadows[k], saved[k]) for k in TRACKED)          # a refused load changes nothing


def test_applied_exchanges_and_restores_bit_for_bit():
    from segland_amd import functional
    from segland_amd.ema import ModelEma
    model = _tiny()
    ema = ModelEma(model, 0.9)
    for t in range(3):
        _perturb(model, 10 + t)
        ema.update()
    live = model.state_dict(keep_vars=True)
    raw = {k: v.detach().clone() for k, v in live.items()}
    avg = {k: v.clone() for k, v in ema.shadows.items()}
    ptrs = {k: v.data_ptr() for k, v in live.items()}
    epochs = (functional._OPT_EPOCH[0], functional._RS_EPOCH[0])
    with ema.applied() as inside:
        assert inside is ema
        assert (functional._OPT_EPOCH[0], functional._RS_EPOCH[0]) == (epochs[0] + 1, epochs[1] + 1)
        for k, v in live.items():
            assert torch.equal(v, avg[k] if k in avg else raw[k]), k
        assert all(torch.equal(ema.shadows[k], raw[k]) for k in TRACKED)
    assert (functional._OPT_EPOCH[0], functional._RS_EPOCH[0]) == (epochs[0] + 2, epochs[1] + 2)
    for k, v in live.items():
        assert torch.equal(v, raw[k]) and v.data_ptr() == ptrs[k], k
    assert all(torch.equal(ema.shadows[k], avg[k]) for k in TRACKED)
    with pytest.raises(ZeroDivisionError):                 # an exception inside still restores
        with ema.applied():
            1 / 0
    assert all(torch.equal(live[k], raw[k]) for k in live) and all(torch.equal(ema.shadows[k], avg[k]) for k in TRACKED)


def test_model_state_dict_has_exactly_the_models_keys():
    from segland_amd.ema import ModelEma
    model = _tiny()
    ema = ModelEma(model, 0.9)
    _perturb(model, 1)
    ema.update()
    sd, msd = model.state_dict(), ema.model_state_dict()
    assert list(msd) == list(sd)
    for k in sd:
        assert msd[k].shape == sd[k].shape and msd[k].dtype == sd[k].dtype
        if k in TRACKED:
            assert torch.equal(msd[k], ema.shadows[k]) and not torch.equal(msd[k], sd[k]), k
        else:
            assert torch.equal(msd[k], sd[k]), k
    fresh = _tiny()
    fresh.load_state_dict(msd, strict=True)


def test_training_state_round_trips_the_ema(tmp_path, caplog):
    from segland_amd.drivers import load_training_state, save_training_state
    from segland_amd.ema import ModelEma
    model = _tiny()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.1, momentum=0.9)
    ema = ModelEma(model, 0.99)
    for t in range(4):
        _perturb(model, 20 + t)
        ema.update()
    with_ema, without = str(tmp_path / 'state_with.pth'), str(tmp_path / 'state_without.pth')
    save_training_state(model, opt, with_ema, 7, best=0.5, best_epoch=6, ema=ema)
    save_training_state(model, opt, without, 7, best=0.5, best_epoch=6)
    ck = torch.load(with_ema, map_location='cpu')
    assert ck['ema']['updates'] == 4 and list(ck['ema']['shadows']) == TRACKED and 'ema' not in torch.load(without, map_location='cpu')
    assert all(torch.equal(ck['state_dict'][k], model.state_dict()[k]) for k in ck['state_dict'])            # the raw weights

    model2 = _tiny()
    _perturb(model2, 99)
    opt2 = torch.optim.SGD([p for p in model2.parameters() if p.requires_grad], lr=0.1, momentum=0.9)
    ema2 = ModelEma(model2, 0.5, warmup=False)
    assert load_training_state(model2, opt2, with_ema, ema=ema2) == (7, 0.5, 6)
    assert (ema2.updates, ema2.decay, ema2.warmup) == (4, 0.99, True)
    assert all(torch.equal(ema2.shadows[k], ema.shadows[k]) for k in TRACKED)
    assert load_training_state(_tiny(), opt2, with_ema) == (7, 0.5, 6)                                   # a run without the flag reads the file as before

    # a state written without the flag: warning, the average starts from the loaded weights
    ema3 = ModelEma(model2, 0.9)
    ema3.updates = 11
    with caplog.at_level(logging.WARNING, logger='Segmentation'):
        load_training_state(model2, opt2, without, ema=ema3)
    assert any('no weight average' in r.getMessage() and without in r.getMessage() for r in caplog.records)
    live = model2.state_dict(keep_vars=True)
    assert ema3.updates == 0 and all(torch.equal(ema3.shadows[k], live[k]) and torch.equal(live[k], model.state_dict()[k]) for k in TRACKED)
