"""Every route of the pyramid-pooling kernels (csrc/ppm.hip) and of the layout kernels that feed them (csrc/conv_weight_prep.hip), through segland_amd.ops, against the
float64 references of tests/ppm_reference.py on the kernel's own (rounded) inputs, inside the derived elementwise bounds stated there.  The case tables, with the
dispatch condition of every route, live in ppm_reference.py; tests/test_ppm_reference_cpu.py checks those conditions, the references and the comparators' sharpness
without a GPU.  Each test prints its worst error / bound ratio (SEGLAND_PARITY_LOG collects them: profiles/parity_ppm.txt)."""
import pytest
import torch

import ppm_reference as pr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DT = sorted(pr.DTYPES)
_cache = {}


def cached(key, make):
    """References and inputs are built once per key, shared and never modified."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def cpu(t):
    return t.detach().cpu()


# ------------------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize('d', DT)
@pytest.mark.parametrize('name', sorted(pr.POOL_FWD_CASES))
def test_pool_forward(hip, name, d):
    """ppm_cells_kernel<T> / ppm_cells_rows_kernel + ppm_bins_kernel: one fp32 ulp of F.adaptive_avg_pool2d on exact integer inputs."""
    from segland_amd import ops
    shape, sizes, routes = pr.POOL_FWD_CASES[name]
    dtype = pr.DTYPES[d]
    assert pr.pool_fwd_route(dtype, *shape, sizes) == routes[d]
    x = cached(('pool/x', name, d), lambda: pr.pool_input('pool/' + name, shape, dtype))
    pr.check_pool_input(x, sizes)                                          # on the reference alone, before anything is launched
    ref = cached(('pool/ref', name), lambda: pr.pool_fwd(x, sizes))
    got = ops.ppm_pool_fwd(x.to(DEV), sizes)
    assert got.dtype == torch.float32 and tuple(got.shape) == (pr.rows(shape[0], sizes), shape[3])
    assert pr.worst_ratio('pool forward %s %s [%s]' % (name, d, routes[d]), cpu(got), ref, pr.pool_fwd_bound(ref)) <= 1


@pytest.mark.parametrize('d', DT)
@pytest.mark.parametrize('cat', sorted(pr.POOL_BWD_DCAT))
@pytest.mark.parametrize('name', sorted(pr.POOL_BWD_CASES))
def test_pool_backward(hip, name, cat, d):
    """ppm_pool_bwd_cells_kernel (wave / scalar route) + ppm_pool_bwd_kernel<T>, with and without the concat slice."""
    from segland_amd import ops
    shape, sizes, route = pr.POOL_BWD_CASES[name]
    B, H, W, C = shape
    dtype, cat_off = pr.DTYPES[d], pr.POOL_BWD_DCAT[cat]
    assert pr.pool_bwd_route(C, sizes) == route
    dp = cached(('pb/dp', name), lambda: pr.randn('pb/dp/' + name, (pr.rows(B, sizes), C)))
    dcat = None
    if cat_off is not None:
        pitch = cat_off + C + 24
        assert pitch > cat_off + C and pitch % 8 == 0
        dcat = cached(('pb/dcat', name, cat, d), lambda: pr.randn('pb/dcat/%s/%s' % (name, cat), (B, H, W, pitch), dtype))
    ref, ref_abs = cached(('pb/ref', name, cat, d), lambda: (pr.pool_bwd(dp, shape, sizes, dcat, cat_off or 0),
                                                              pr.pool_bwd(dp.abs(), shape, sizes, None if dcat is None else dcat.abs(), cat_off or 0)))
    got = ops.ppm_pool_bwd(dp.to(DEV), shape, dtype, sizes, dcat=None if dcat is None else dcat.to(DEV), cat_off=cat_off or 0)
    assert got.dtype == dtype and tuple(got.shape) == shape
    assert pr.worst_ratio('pool backward %s dcat %s %s' % (name, cat, d), cpu(got), ref, pr.pool_bwd_bound(ref, ref_abs, dtype)) <= 1


# ------------------------------------------------------------------------------------------------------------ upsample
def _upsample_case(name, Cs):
    B, H, W = pr.UPSAMPLE_MAPS[name]
    return B, H, W, (B, H, W, 2 * Cs)


@pytest.mark.parametrize('d', DT)
@pytest.mark.parametrize('Cs', pr.UPSAMPLE_CS)
@pytest.mark.parametrize('name', sorted(pr.UPSAMPLE_MAPS))
def test_upsample_forward(hip, name, Cs, d):
    """ppm_upsample_fwd_kernel<T> against F.interpolate(bilinear, align_corners=False)."""
    from segland_amd import ops
    B, H, W, shape = _upsample_case(name, Cs)
    dtype, sizes = pr.DTYPES[d], pr.SIZES
    stage = cached(('up/stage', name, Cs), lambda: pr.randn('up/%s/%d' % (name, Cs), (pr.rows(B, sizes), Cs)))
    ref, ref_abs = cached(('up/ref', name, Cs), lambda: (pr.upsample_fwd(stage, shape, sizes), pr.upsample_fwd(stage.abs(), shape, sizes)))
    got = ops.ppm_upsample_fwd(stage.to(DEV), shape, sizes, dtype)
    assert got.dtype == dtype and tuple(got.shape) == (B, H, W, 4 * Cs)
    assert pr.worst_ratio('upsample forward %s Cs %d %s' % (name, Cs, d), cpu(got), ref, pr.bilinear_bound(ref, ref_abs, dtype)) <= 1


@pytest.mark.parametrize('d', DT)
@pytest.mark.parametrize('Cs', pr.UPSAMPLE_CS)
@pytest.mark.parametrize('name', sorted(pr.UPSAMPLE_MAPS))
def test_upsample_backward(hip, name, Cs, d):
    """ppm_upsample_bwd_x_kernel<T> + ppm_upsample_bwd_y_kernel against the autograd of F.interpolate; the gradient's pitch is wider than the four priors."""
    from segland_amd import ops
    B, H, W, shape = _upsample_case(name, Cs)
    dtype, sizes = pr.DTYPES[d], pr.SIZES
    dcat = cached(('upb/dcat', name, Cs, d), lambda: pr.randn('upb/%s/%d' % (name, Cs), (B, H, W, 4 * Cs + 8), dtype))
    ref, ref_abs = cached(('upb/ref', name, Cs, d), lambda: (pr.upsample_bwd(dcat, shape, sizes, Cs), pr.upsample_bwd(dcat.abs(), shape, sizes, Cs)))
    got = ops.ppm_upsample_bwd(dcat.to(DEV), shape, sizes, Cs)
    assert got.dtype == torch.float32
    assert pr.worst_ratio('upsample backward %s Cs %d %s' % (name, Cs, d), cpu(got), ref, pr.bilinear_bound(ref, ref_abs)) <= 1


# ------------------------------------------------------------------------------------------------------------ factorised prior gather / scatter
def _fact_case(name, d):
    (B, H, W), ns, hook, routes = pr.FACT_CASES[name]
    dtype, N = pr.DTYPES[d], ns[d]
    assert pr.scatter_route(dtype, H, W, N, pr.SIZES, hook) == routes[d]
    return B, H, W, N, dtype, hook, routes[d], (B, H, W, 2048)


@pytest.mark.parametrize('d', DT)
@pytest.mark.parametrize('name', sorted(pr.FACT_CASES))
def test_fact_gather(hip, name, d):
    """ppm_fact_gather1_kernel + ppm_fact_gather2_kernel<T> against the float64 sum over taps and cells (= conv3x3 of the upsampled maps, test_ppm_reference_cpu.py)."""
    from segland_amd import ops
    B, H, W, N, dtype, hook, _, shape = _fact_case(name, d)
    sizes = pr.SIZES
    q = cached(('fact/q', name, N), lambda: pr.randn('fact/q/' + name, (pr.rows(B, sizes), 9 * N)))
    ref, ref_abs = cached(('fact/gref', name, N), lambda: (pr.fact_gather(q, shape, sizes, N), pr.fact_gather(q.abs(), shape, sizes, N)))
    if not hook:
        hip.sl_debug_ppm_fact_walk(0)                                      # conftest's _reset_debug_hooks puts it back
    got = ops.ppm_fact_gather(q.to(DEV), shape, sizes, N, dtype)
    assert got.dtype == dtype and tuple(got.shape) == (B, H, W, N)
    assert pr.worst_ratio('gather %s N %d %s' % (name, N, d), cpu(got), ref, pr.bilinear_bound(ref, ref_abs, dtype)) <= 1


@pytest.mark.parametrize('d', DT)
@pytest.mark.parametrize('name', sorted(pr.FACT_CASES))
def test_fact_scatter(hip, name, d):
    """ppm_fact_scatterA2/B2_kernel (walk) or ppm_fact_scatterA/B_kernel (general, wave / scalar stages) against the exact transpose of the gather in float64."""
    from segland_amd import ops
    B, H, W, N, dtype, hook, route, shape = _fact_case(name, d)
    sizes = pr.SIZES
    dcb = cached(('fact/d', name, N, d), lambda: pr.randn('fact/d/' + name, (B, H, W, N), dtype))
    ref, ref_abs = cached(('fact/sref', name, N, d), lambda: (pr.fact_scatter(dcb, shape, sizes), pr.fact_scatter(dcb.abs(), shape, sizes)))
    if not hook:
        hip.sl_debug_ppm_fact_walk(0)
    got = ops.ppm_fact_scatter(dcb.to(DEV), shape, sizes)
    assert got.dtype == torch.float32 and tuple(got.shape) == (pr.rows(B, sizes), 9 * N)
    assert pr.worst_ratio('scatter %s N %d %s [%s]' % (name, N, d, route), cpu(got), ref, pr.bilinear_bound(ref, ref_abs)) <= 1


# ------------------------------------------------------------------------------------------------------------ stage BatchNorm + ReLU backward, rows weight gradient
@pytest.mark.parametrize('name', sorted(pr.STAGE_BN_CASES))
def test_stage_bn_backward(hip, name):
    """ppm_stage_bn_bwd_kernel against the float64 closed form (the autograd of relu(batch_norm), test_ppm_reference_cpu.py): dx, dgamma, dbeta to 1e-5 of each tensor's
    maximum per level (a one-row level in train mode, whose gradient is 0 identically: ppm_reference.stage_bn_dx_bound).  At B = 16 the 6x6 level takes five 128-row
    trips, the last one ragged (64 rows)."""
    from segland_amd import ops
    B, C, trains, no_gamma = pr.STAGE_BN_CASES[name]
    sizes = pr.SIZES
    x, dy, y, means, invs, gammas = pr.stage_bn_inputs('bn/' + name, B, C, sizes, trains, no_gamma)
    rdx, rdg, rdb = pr.stage_bn_bwd(dy, y, x, B, sizes, means, invs, gammas, trains)
    dev = lambda ts: [None if t is None else t.to(DEV) for t in ts]
    dg = [torch.full((C,), float('nan'), device=DEV) for _ in sizes]
    db = [torch.full((C,), float('nan'), device=DEV) for _ in sizes]
    dx = ops.ppm_stage_bn_bwd(dy.to(DEV), y.to(DEV), x.to(DEV), B, sizes, dev(means), dev(invs), dev(gammas), trains, dg, db)
    worst = 0.0
    for l, sl in enumerate(pr.level_slices(B, sizes)):
        tag = 'stage bn %s level %d (%d rows, %s)' % (name, l, sl.stop - sl.start, 'train' if trains[l] else 'eval')
        worst = max(worst, pr.worst_ratio(tag + ' dx', cpu(dx)[sl], rdx[sl], pr.stage_bn_dx_bound(rdx[sl], dy[sl], y[sl], invs[l], gammas[l], trains[l])),
                    pr.worst_ratio(tag + ' dgamma', cpu(dg[l]), rdg[l], pr.max_bound(rdg[l])),
                    pr.worst_ratio(tag + ' dbeta', cpu(db[l]), rdb[l], pr.max_bound(rdb[l])))
    assert worst <= 1


@pytest.mark.parametrize('name', sorted(pr.ROWS_WGRAD_CASES))
def test_rows_weight_gradient(hip, name):
    """ppm_rows_wgrad_kernel against the float64 einsum per level at 1e-5 of its maximum; at B = 1 the first level is one row inside a 32-row chunk."""
    from segland_amd import ops
    B, N, K = pr.ROWS_WGRAD_CASES[name]
    sizes = pr.SIZES
    a, x = pr.randn('rw/a/' + name, (pr.rows(B, sizes), N)), pr.randn('rw/x/' + name, (pr.rows(B, sizes), K))
    ref = pr.rows_wgrad(a, x, B, sizes)
    got = ops.ppm_rows_wgrad(a.to(DEV), x.to(DEV), B, sizes)
    worst = max(pr.worst_ratio('rows wgrad %s level %d' % (name, l), cpu(got[l]).view(N, K), ref[l], pr.max_bound(ref[l])) for l in range(len(sizes)))
    assert worst <= 1


# ------------------------------------------------------------------------------------------------------------ layout kernels, bit for bit
@pytest.mark.parametrize('name', sorted(pr.WQ_CASES))
def test_wq_prep_and_dwq_scatter(hip, name):
    """ppm_wq_prep_tiles_kernel and ppm_dwq_scatter_kernel against torch indexing; the columns of dw beyond the nl slices stay untouched."""
    from segland_amd import ops
    N, Cs, nl, Ctot = pr.WQ_CASES[name]
    w = pr.randn('wq/' + name, (N, Ctot, 3, 3))
    rf, rb = pr.wq_layouts(w, Cs, nl)
    wq_f, wq_b = ops.ppm_wq_prep(w.to(DEV), Cs, nl)
    assert torch.equal(cpu(wq_f), rf) and torch.equal(cpu(wq_b), rb)
    dwq = pr.randn('dwq/' + name, (nl, 9 * N, Cs))
    dw0 = pr.randn('dw0/' + name, (N, Ctot, 3, 3))
    dw = dw0.to(DEV)
    ops.ppm_dwq_scatter(dwq.to(DEV), dw, Cs, nl)
    assert torch.equal(cpu(dw), pr.dwq_scatter(dwq, dw0, Cs, nl))
    if nl * Cs < Ctot:
        assert torch.equal(cpu(dw)[:, nl * Cs:], dw0[:, nl * Cs:])
    print('wq prep / dwq scatter %s: bit-identical' % name)


@pytest.mark.parametrize('d', DT)
@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('name', sorted(pr.SLICE_CASES))
def test_weight_prep_slice(hip, name, k, d):
    """weight_prep_slice_tiles_kernel (tiled) / weight_prep_slice_kernel<T> (scalar) against permute of the sliced OIHW weight, rounded once."""
    from segland_amd import ops
    O, cin, off, cnt, route = pr.SLICE_CASES[name]
    dtype = pr.DTYPES[d]
    assert pr.slice_route(O, off, cnt, k * k) == route
    w = cached(('slice/w', name, k), lambda: pr.randn('slice/%s/%d' % (name, k), (O, cin, k, k)))
    rf, rb = pr.slice_layouts(w, dtype, off, cnt)
    wf, wb = ops.weight_prep_slice(w.to(DEV), dtype, off, cnt)
    assert wf.dtype == wb.dtype == dtype
    assert torch.equal(cpu(wf), rf) and torch.equal(cpu(wb), rb)
    print('weight_prep_slice %s %dx%d %s [%s]: bit-identical' % (name, k, k, d, route))
