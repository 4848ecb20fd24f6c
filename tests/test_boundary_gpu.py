"""Boundary IoU and trimap counts on the GPU (sl_boundary_counts -> ops.boundary_counts -> eval_base --boundary-width): both outputs bit for bit against the numpy
contract of tests/boundary_reference.py (integer counts: no tolerance), accumulation, run-to-run determinism, batch isolation, and the evaluation drivers.  Without
the entry point, the op and the flag every test here fails."""
import numpy as np
import pytest
import torch

import boundary_reference as br
from eval_common import run_eval

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def device_maps(name):
    pred, target = br.case_maps(name)
    return torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV)


def as_tensors(ref):
    return torch.from_numpy(ref[0]), torch.from_numpy(ref[1])


@pytest.mark.parametrize('name', list(br.CASES))
def test_counts_equal_the_reference(hip, name):
    """torch.equal on counts [3][K] and band_cm [K][K].  The reference's own bands cover strictly between 0 and 100 % of the map (asserted here, on the reference), so
    a broken interior test cannot hide behind a map that is all band; the case with H < d is all band on purpose and checks saturation."""
    from segland_amd import ops
    (B, H, W, K, d), _, saturating, _ = br.CASES[name]
    ref_counts, ref_cm, g, p = br.case_reference(name)
    assert (g == 1.0 and p == 1.0) if saturating else (0.0 < g < 1.0 and 0.0 < p < 1.0), (g, p)
    assert ref_counts[1].sum() > 0 and ref_counts[0].sum() > 0 and ref_cm.sum() > 0
    pred, target = device_maps(name)
    counts, band_cm = ops.boundary_counts(pred, target, K, br.IGNORE_INDEX, d)
    assert counts.dtype == torch.int64 and counts.shape == (3, K) and band_cm.dtype == torch.int64 and band_cm.shape == (K, K)
    want_counts, want_cm = as_tensors((ref_counts, ref_cm))
    assert torch.equal(counts.cpu(), want_counts), (counts.cpu() - want_counts)
    assert torch.equal(band_cm.cpu(), want_cm)


def test_second_call_into_the_same_buffers_doubles_them(hip):
    """The entry point ADDS: called twice on the buffers of the first call (through the C ABI, as a driver that accumulates in place would)."""
    from segland_amd import ops
    (B, H, W, K, d) = br.CASES['ragged'][0]
    pred, target = device_maps('ragged')
    counts, band_cm = ops.boundary_counts(pred, target, K, br.IGNORE_INDEX, d)
    once = counts.clone(), band_cm.clone()
    ops.check(hip.sl_boundary_counts(pred.data_ptr(), target.data_ptr(), B, H, W, K, br.IGNORE_INDEX, d, counts.data_ptr(), band_cm.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), 'boundary_counts')
    assert torch.equal(counts, 2 * once[0]) and torch.equal(band_cm, 2 * once[1]) and once[0].sum() > 0


@pytest.mark.parametrize('name', ['ragged', 'lds'])
def test_two_runs_give_the_same_counts(hip, name):
    from segland_amd import ops
    (B, H, W, K, d) = br.CASES[name][0]
    pred, target = device_maps(name)
    a, b = ops.boundary_counts(pred, target, K, br.IGNORE_INDEX, d), ops.boundary_counts(pred, target, K, br.IGNORE_INDEX, d)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('name', ['ragged', 'row129'])
def test_batch_is_the_sum_of_its_images(hip, name):
    """B = 2: nothing bleeds from one image's halo into the next image of the batch."""
    from segland_amd import ops
    (B, H, W, K, d) = br.CASES[name][0]
    assert B == 2
    pred, target = device_maps(name)
    both = ops.boundary_counts(pred, target, K, br.IGNORE_INDEX, d)
    one = [ops.boundary_counts(pred[b:b + 1].contiguous(), target[b:b + 1].contiguous(), K, br.IGNORE_INDEX, d) for b in range(2)]
    assert torch.equal(both[0], one[0][0] + one[1][0]) and torch.equal(both[1], one[0][1] + one[1][1])
    assert one[0][0].sum() > 0 and one[1][0].sum() > 0


def recorded_eval(out, monkeypatch, ft):
    """eval_base with --boundary-width 3 and ops.boundary_counts wrapped by a recorder -> (cmatrix, bcounts, band_cmatrix as saved, reference sums over the batches)."""
    import os
    from segland_amd import ops
    real, seen = ops.boundary_counts, []

    def recorder(pred, label, K, ignore_index, d):
        seen.append((pred.cpu().numpy().copy(), label.cpu().numpy().copy(), K, ignore_index, d))
        return real(pred, label, K, ignore_index, d)
    monkeypatch.setattr(ops, 'boundary_counts', recorder)
    cm = run_eval(out, ['--boundary-width', '3'], ft=ft)
    monkeypatch.setattr(ops, 'boundary_counts', real)
    assert seen and all(s[4] == 3 for s in seen)
    want_counts, want_cm = 0, 0
    for pred, label, K, ignore_index, d in seen:
        c, m, _, _ = br.contract_counts(pred, label, K, ignore_index, d)
        want_counts, want_cm = want_counts + c, want_cm + m
    return cm, np.load(os.path.join(str(out), 'bcounts_123.npy')), np.load(os.path.join(str(out), 'band_cmatrix_123.npy')), want_counts, want_cm


def test_eval_driver_with_boundary_width(hip, tmp_path, monkeypatch):
    """cmatrix_123.npy is bit-equal with and without the flag; the saved boundary files are the numpy reference summed over the (pred, label) batches the driver
    handed to the op; the six log lines are written; without the flag the op is not called and no boundary file appears."""
    import glob
    import os
    from segland_amd import ops

    def refuse(*a, **k):
        raise AssertionError('ops.boundary_counts called')
    monkeypatch.setattr(ops, 'boundary_counts', refuse)
    plain = run_eval(tmp_path / 'plain', [])
    monkeypatch.undo()
    assert not os.path.exists(str(tmp_path / 'plain' / 'bcounts_123.npy')) and not os.path.exists(str(tmp_path / 'plain' / 'band_cmatrix_123.npy'))
    cm, bcounts, band_cm, want_counts, want_cm = recorded_eval(tmp_path / 'on', monkeypatch, ft=False)
    assert np.array_equal(cm, plain) and cm.sum() > 0
    assert bcounts.shape == (3, 12) and np.array_equal(bcounts, want_counts) and want_counts[1].sum() > 0
    assert band_cm.shape == (12, 12) and np.array_equal(band_cm, want_cm) and (band_cm <= cm).all()
    log = ''.join(open(f).read() for f in glob.glob(str(tmp_path / 'on' / '*.log')))
    for name in ('boundaryIoU', 'trimapIoU'):
        for part in ('base', 'novel', 'total'):
            assert '%s(d=3)---%s: mIoU ' % (name, part) in log, (name, part)


def test_eval_ft_driver_with_boundary_width(hip, tmp_path, monkeypatch):
    """The same through the eval_ft call, whose labels are padded with ignore to a square of their long side before they reach the op."""
    plain = run_eval(tmp_path / 'plain', [], ft=True)
    cm, bcounts, band_cm, want_counts, want_cm = recorded_eval(tmp_path / 'on', monkeypatch, ft=True)
    assert np.array_equal(cm, plain) and cm.sum() > 0
    assert np.array_equal(bcounts, want_counts) and np.array_equal(band_cm, want_cm) and want_counts[1].sum() > 0
