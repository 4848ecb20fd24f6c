"""tests/ppm_reference.py checked on the CPU alone: the float64 references against independent torch evaluations (conv2d of the upsampled maps, autograd, explicit loops),
the input conditions the comparators rest on, the dispatch route of every case of tests/test_ppm_parity_gpu.py, and the sharpness of the comparators -- each one must
reject a reference perturbed the way a subtly wrong kernel would be (a pixel dropped from a bin, an unmasked border tap, align_corners=True weights, a source cell off
by one, one level's rows offset by one)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import ppm_reference as pr

F64 = torch.float64
BOTH = (torch.float32, torch.bfloat16)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------ routes and input conditions
def test_every_case_reaches_the_route_its_id_names():
    for name, (shape, sizes, routes) in pr.POOL_FWD_CASES.items():
        for d, route in routes.items():
            assert pr.pool_fwd_route(pr.DTYPES[d], *shape, sizes) == route, (name, d)
    assert (pr.cell_count(pr.SIZES, 13), pr.cell_count(pr.SIZES, 22)) == (11, 10)
    assert 8 * 11 * 11 * 256 == 247808 < 262144 <= 9 * 11 * 11 * 256 == 278784
    assert {r for _, _, rt in pr.POOL_FWD_CASES.values() for r in rt.values()} == {'rows', 'cells'}
    for name, (shape, sizes, route) in pr.POOL_BWD_CASES.items():
        assert pr.pool_bwd_route(shape[3], sizes) == route and route in name, name
    assert sum(s * s for s in (1, 2, 3, 8)) == 78
    for name, (shape, ns, hook, routes) in pr.FACT_CASES.items():
        for d, route in routes.items():
            assert pr.scatter_route(pr.DTYPES[d], shape[1], shape[2], ns[d], pr.SIZES, hook) == route, (name, d)
    # the case the hook sends to the general kernels would walk without it
    assert pr.scatter_route(torch.float32, 66, 6, 64, pr.SIZES, True) == 'walk'
    assert {r for *_, rt in pr.FACT_CASES.values() for r in rt.values()} == {
        'walk', 'general:A-scalar:B-scalar', 'general:A-scalar:B-wave', 'general:A-wave:B-wave'}
    assert pr.stage_bn_trips(16, 6) == (5, 64) and pr.stage_bn_trips(16, 3) == (2, 16) and pr.stage_bn_trips(1, 1) == (1, 1) and pr.stage_bn_trips(5, 6) == (2, 52)
    assert pr.STAGE_BN_CASES['b16-c96-five-trips'][1] // 32 == 3
    for name, (O, cin, off, cnt, route) in pr.SLICE_CASES.items():
        for taps in (1, 9):
            assert pr.slice_route(O, off, cnt, taps) == route, name
        assert off + cnt <= cin


@pytest.mark.parametrize('dtype', BOTH)
@pytest.mark.parametrize('name', sorted(pr.POOL_FWD_CASES))
def test_pool_inputs_meet_the_exactness_conditions(name, dtype):
    shape, sizes, _ = pr.POOL_FWD_CASES[name]
    x = pr.pool_input('pool/' + name, shape, dtype)
    assert bool((x.to(F64) == pr.pool_input('pool/' + name, shape, torch.float32).to(F64)).all())      # exact in bf16
    pr.check_pool_input(x, sizes)
    if x.numel() >= 64:
        assert sorted(x.to(F64).unique().tolist()) == [-3, -2, -1, 0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------------------ references against independent evaluations
@pytest.mark.parametrize('H,W', [(5, 4), (13, 22), (1, 1)])
def test_bin_matrices_reproduce_adaptive_pooling(H, W):
    """bin_membership / bin_area (used for the exactness check and the perturbations) give adaptive_avg_pool2d back."""
    x = pr.randn('cpu/bins', (2, H, W, 3)).to(F64)
    ref = pr.pool_fwd(x, pr.SIZES)
    for sl, s in zip(pr.level_slices(2, pr.SIZES), pr.SIZES):
        mine = torch.einsum('iy,jx,byxc->bijc', pr.bin_membership(s, H), pr.bin_membership(s, W), x) / pr.bin_area(s, H, W)[None, :, :, None]
        assert rel(mine.reshape(-1, 3), ref[sl]) <= 1e-14


@pytest.mark.parametrize('shape', [(2, 5, 4, 8), (2, 13, 22, 8)])
def test_pool_backward_is_the_transpose_plus_the_concat_slice(shape):
    B, H, W, C = shape
    x = pr.randn('cpu/pb/x', shape).to(F64)
    dp = pr.randn('cpu/pb/dp', (pr.rows(B, pr.SIZES), C))
    dcat = pr.randn('cpu/pb/dcat', (B, H, W, C + 24))
    lhs = float((pr.pool_fwd(x, pr.SIZES) * dp.to(F64)).sum())
    rhs = float((x * pr.pool_bwd(dp, shape, pr.SIZES)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    both = pr.pool_bwd(dp, shape, pr.SIZES, dcat, 16)
    assert rel(both - pr.pool_bwd(dp, shape, pr.SIZES), dcat.to(F64)[..., 16:16 + C]) <= 1e-14


@pytest.mark.parametrize('H,W', [(5, 4), (6, 6), (13, 22), (1, 1)])
def test_interpolation_matrices_reproduce_interpolate(H, W):
    shape = (2, H, W, 8)
    stage = pr.randn('cpu/up', (pr.rows(2, pr.SIZES), 8))
    ref = pr.upsample_fwd(stage, shape, pr.SIZES)
    assert rel(pr.upsample_fwd_mat(stage, shape, pr.SIZES), ref) <= 1e-12
    for s in pr.SIZES:
        u = pr.interp_matrix(s, H)
        assert float((u.sum(1) - 1).abs().max()) <= 1e-14 and float(u.min()) >= 0          # non-negative weights: R_abs bounds the sum of |terms|
    dcat = pr.randn('cpu/up/d', (2, H, W, 4 * 8 + 16))
    lhs = float((ref * dcat.to(F64)[..., :32]).sum())
    rhs = float((stage.to(F64) * pr.upsample_bwd(dcat, shape, pr.SIZES, 8)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    if (H, W) == (6, 6):
        assert torch.equal(pr.interp_matrix(6, 6), torch.eye(6, dtype=F64))                # the 6x6 level is the identity there


@pytest.mark.parametrize('B,H,W,Cs,N', [(2, 5, 9, 4, 6), (2, 5, 4, 4, 6), (1, 7, 6, 2, 3)])
def test_gather_is_conv3x3_of_the_upsampled_maps(B, H, W, Cs, N):
    """fact_gather(q) with q_l = P_l x W_l equals F.conv2d(cat_l interpolate(P_l), W, padding=1) to 1e-12."""
    sizes, nl = pr.SIZES, len(pr.SIZES)
    shape = (B, H, W, 8)
    stage = pr.randn('cpu/g/stage', (pr.rows(B, sizes), Cs)).to(F64)
    w = pr.randn('cpu/g/w', (N, nl * Cs, 3, 3)).to(F64)
    ups = pr.upsample_fwd(stage, shape, sizes).permute(0, 3, 1, 2)
    ref = F.conv2d(ups, w, padding=1).permute(0, 2, 3, 1)
    wq_f, wq_b = pr.wq_layouts(w, Cs, nl)
    q = torch.cat([stage[sl] @ wq_f[l].t() for l, sl in enumerate(pr.level_slices(B, sizes))], 0)
    got = pr.fact_gather(q, shape, sizes, N)
    err = float((got - ref).abs().max())
    print('gather vs conv2d(upsample) at %s: %.3g' % ((B, H, W, Cs, N), err))
    assert err <= 1e-12
    assert torch.equal(wq_b, wq_f.transpose(1, 2))


@pytest.mark.parametrize('B,H,W,N', [(2, 5, 9, 6), (2, 5, 4, 6), (1, 66, 6, 2)])
def test_scatter_is_the_autograd_of_the_gather(B, H, W, N):
    sizes, shape = pr.SIZES, (B, H, W, 8)
    q = pr.randn('cpu/s/q', (pr.rows(B, sizes), 9 * N)).to(F64).requires_grad_(True)
    d = pr.randn('cpu/s/d', (B, H, W, N))
    g, = torch.autograd.grad(pr.fact_gather(q, shape, sizes, N), q, d.to(F64))
    assert float((pr.fact_scatter(d, shape, sizes) - g).abs().max()) <= 1e-12


@pytest.mark.parametrize('B', [2, 5])
def test_stage_bn_closed_form_is_the_autograd_of_relu_batch_norm(B):
    sizes, C, trains = pr.SIZES, 8, (True, False, True, True)
    x, dy, y, means, invs, gammas = pr.stage_bn_inputs('cpu/bn%d' % B, B, C, sizes, trains, no_gamma=(3,))
    means64, invs64, y64 = [], [], torch.empty(x.shape, dtype=F64)
    auto = []
    for l, sl in enumerate(pr.level_slices(B, sizes)):
        xl = x[sl].to(F64).requires_grad_(True)
        gm = (gammas[l].to(F64) if gammas[l] is not None else torch.ones(C, dtype=F64)).requires_grad_(True)
        beta = torch.full((C,), 0.1, dtype=F64, requires_grad=True)
        if trains[l]:
            m, v = xl.detach().mean(0), xl.detach().var(0, unbiased=False)
            out = torch.relu(F.batch_norm(xl, None, None, gm, beta, training=True, eps=1e-5))
        else:
            m, v = means[l].to(F64), invs[l].to(F64) ** -2 - 1e-5
            out = torch.relu(F.batch_norm(xl, m, v, gm, beta, training=False, eps=1e-5))
        means64.append(m); invs64.append((v + 1e-5).rsqrt()); y64[sl] = out.detach()
        auto.append(torch.autograd.grad(out, (xl, gm, beta), dy[sl].to(F64)))
    dx, dgs, dbs = pr.stage_bn_bwd(dy, y64, x, B, sizes, means64, invs64, gammas, trains)
    for l, sl in enumerate(pr.level_slices(B, sizes)):
        assert rel(dx[sl], auto[l][0]) <= 1e-10 and rel(dgs[l], auto[l][1]) <= 1e-10 and rel(dbs[l], auto[l][2]) <= 1e-10, l
    # the generator's fp32 y gates the same elements as the float64 forward away from y == 0
    assert float(((y > 0) != (y64 > 0)).double().mean()) <= 1e-3


def test_layout_references_by_explicit_loops():
    N, Cs, nl, Ctot = 4, 3, 2, 8
    w = pr.randn('cpu/wq', (N, Ctot, 3, 3))
    wq_f, wq_b = pr.wq_layouts(w, Cs, nl)
    dw0 = pr.randn('cpu/dw', (N, Ctot, 3, 3))
    dw = pr.dwq_scatter(wq_f, dw0, Cs, nl)
    for l in range(nl):
        for tap in range(9):
            for n in range(N):
                for c in range(Cs):
                    v = w[n, l * Cs + c, tap // 3, tap % 3]
                    assert wq_f[l, tap * N + n, c] == v and wq_b[l, c, tap * N + n] == v and dw[n, l * Cs + c, tap // 3, tap % 3] == v
    assert torch.equal(dw[:, nl * Cs:], dw0[:, nl * Cs:])
    for dtype in BOTH:
        wf, wb = pr.slice_layouts(w, dtype, 2, 5)
        assert wf.dtype == wb.dtype == dtype and wf.shape == (N, 3, 3, 5) and wb.shape == (5, 3, 3, N)
        for o in range(N):
            for i in range(5):
                assert torch.equal(wf[o, :, :, i], w[o, 2 + i].to(dtype)) and torch.equal(wb[i, :, :, o], w[o, 2 + i].to(dtype))


# ------------------------------------------------------------------------------------------------------------ the bilinear bound is neither vacuous nor knife-edge
@pytest.mark.parametrize('Cs', pr.UPSAMPLE_CS)
@pytest.mark.parametrize('name', sorted(pr.UPSAMPLE_MAPS))
def test_torch_fp32_interpolate_stays_inside_a_quarter_of_the_bilinear_bound(name, Cs):
    B, H, W = pr.UPSAMPLE_MAPS[name]
    sizes, shape = pr.SIZES, (B, H, W, 2 * Cs)
    stage = pr.randn('up/%s/%d' % (name, Cs), (pr.rows(B, sizes), Cs))
    dcat = pr.randn('upb/%s/%d' % (name, Cs), (B, H, W, 4 * Cs + 8))
    ref, ref_abs = pr.upsample_fwd(stage, shape, sizes), pr.upsample_fwd(stage.abs(), shape, sizes)
    st = stage.clone().requires_grad_(True)
    out32 = torch.cat([F.interpolate(m, size=(H, W), mode='bilinear', align_corners=False) for m in pr.to_maps(st, B, sizes)], 1).permute(0, 2, 3, 1)
    assert out32.dtype == torch.float32
    assert pr.worst_ratio('torch fp32 upsample %s Cs %d' % (name, Cs), out32.detach(), ref, pr.bilinear_bound(ref, ref_abs) / 4) <= 1
    g32, = torch.autograd.grad(out32, st, dcat[..., :4 * Cs])
    bref, bref_abs = pr.upsample_bwd(dcat, shape, sizes, Cs), pr.upsample_bwd(dcat.abs(), shape, sizes, Cs)
    assert pr.worst_ratio('torch fp32 upsample backward %s Cs %d' % (name, Cs), g32, bref, pr.bilinear_bound(bref, bref_abs) / 4) <= 1


# ------------------------------------------------------------------------------------------------------------ sharpness: a subtly wrong kernel is rejected
def _align_corners(s, n):
    return pr.interp_matrix(s, n, align_corners=True)


def _cell_off_by_one(s, n):
    return pr.interp_matrix(s, n).roll(1, dims=1)


def _roll_level(t_rows, B, sizes, level):
    out = t_rows.clone()
    sl = pr.level_slices(B, sizes)[level]
    out[sl] = t_rows[sl].roll(1, dims=0)
    return out


def _first_pixel(s, n, i):
    return int(pr.bin_membership(s, n)[i].nonzero()[0])


def test_pool_comparators_reject_a_dropped_pixel_and_offset_rows():
    shape, sizes, _ = pr.POOL_FWD_CASES['ragged-11x10-cells']
    B, H, W, C = shape
    x = pr.pool_input('pool/ragged-11x10-cells', shape, torch.bfloat16)
    ref = pr.pool_fwd(x, sizes)
    assert pr.worst_ratio('pool: reference against itself', ref, ref, pr.pool_fwd_bound(ref)) == 0
    assert pr.worst_ratio('pool: reference rounded to fp32', ref.float(), ref, pr.pool_fwd_bound(ref)) <= 0.5
    # one pixel missing from bin (1, 1) of the 3x3 level of image 1 (13 and 22 are no multiples of 3)
    lvl, s, b, i, j = 2, 3, 1, 1, 1
    assert H % s and W % s
    row = pr.level_slices(B, sizes)[lvl].start + (b * s + i) * s + j
    y0, x0 = _first_pixel(s, H, i), _first_pixel(s, W, j)
    area = float(pr.bin_area(s, H, W)[i, j])
    bad = ref.clone()
    bad[row] -= x[b, y0, x0].to(F64) / area
    assert pr.worst_ratio('pool: one pixel dropped from a bin', bad, ref, pr.pool_fwd_bound(ref)) > 1e3
    assert pr.worst_ratio('pool: level 2 rows offset by one', _roll_level(ref, B, sizes, 2), ref, pr.pool_fwd_bound(ref)) > 1e3
    # backward: the same bin forgets the same pixel; a level's rows read one row off
    dp = pr.randn('cpu/sharp/dp', (pr.rows(B, sizes), C))
    dcat = pr.randn('cpu/sharp/dcat', (B, H, W, C + 24), torch.bfloat16)
    for dtype in BOTH:
        bref, babs = pr.pool_bwd(dp, shape, sizes, dcat, 0), pr.pool_bwd(dp.abs(), shape, sizes, dcat.abs(), 0)
        bound = pr.pool_bwd_bound(bref, babs, dtype)
        assert pr.worst_ratio('pool backward: reference rounded to %s' % dtype, bref.to(dtype), bref, bound) <= 1
        bad = bref.clone()
        bad[b, y0, x0] -= dp[row].to(F64) / area
        assert pr.worst_ratio('pool backward: one pixel dropped from a bin (%s)' % dtype, bad, bref, bound) > (1e3 if dtype == torch.float32 else 1)
        off = pr.pool_bwd(_roll_level(dp, B, sizes, 3), shape, sizes, dcat, 0)
        assert pr.worst_ratio('pool backward: level 3 rows offset by one (%s)' % dtype, off, bref, bound) > (1e3 if dtype == torch.float32 else 1)
        wrong_slice = pr.pool_bwd(dp, shape, sizes, dcat, 8)
        assert pr.worst_ratio('pool backward: concat slice 8 channels off (%s)' % dtype, wrong_slice, bref, bound) > (1e3 if dtype == torch.float32 else 1)


@pytest.mark.parametrize('name', ['5x4', '13x22', '64x40'])
def test_bilinear_comparator_rejects_wrong_upsampling(name):
    B, H, W = pr.UPSAMPLE_MAPS[name]
    sizes, Cs, shape = pr.SIZES, 8, (B, H, W, 16)
    stage = pr.randn('up/%s/%d' % (name, Cs), (pr.rows(B, sizes), Cs))
    ref, ref_abs = pr.upsample_fwd(stage, shape, sizes), pr.upsample_fwd(stage.abs(), shape, sizes)
    dcat = pr.randn('upb/%s/%d' % (name, Cs), (B, H, W, 4 * Cs + 8))
    bref, babs = pr.upsample_bwd(dcat, shape, sizes, Cs), pr.upsample_bwd(dcat.abs(), shape, sizes, Cs)

    def bwd_mat(interp):
        st = torch.zeros(stage.shape, dtype=F64, requires_grad=True)
        return torch.autograd.grad(pr.upsample_fwd_mat(st, shape, sizes, interp), st, dcat.to(F64)[..., :4 * Cs])[0]
    assert rel(bwd_mat(pr.interp_matrix), bref) <= 1e-12
    for dtype in BOTH:
        fb, bb = pr.bilinear_bound(ref, ref_abs, dtype), pr.bilinear_bound(bref, babs)
        assert pr.worst_ratio('upsample: reference rounded to %s' % dtype, ref.to(dtype), ref, fb) <= 1
        floor = 1e3 if dtype == torch.float32 else 4
        for what, interp in (('align_corners=True weights', _align_corners), ('source cell off by one', _cell_off_by_one)):
            assert pr.worst_ratio('upsample %s: %s (%s)' % (name, what, dtype), pr.upsample_fwd_mat(stage, shape, sizes, interp), ref, fb) > floor
            assert pr.worst_ratio('upsample backward %s: %s' % (name, what), bwd_mat(interp), bref, bb) > 1e3
        bad = pr.upsample_fwd(_roll_level(stage, B, sizes, 1), shape, sizes)
        assert pr.worst_ratio('upsample %s: level 1 rows offset by one (%s)' % (name, dtype), bad, ref, fb) > floor
    bad = bref.clone()
    bad = _roll_level(bad, B, sizes, 3)
    assert pr.worst_ratio('upsample backward %s: level 3 rows offset by one' % name, bad, bref, pr.bilinear_bound(bref, babs)) > 1e3


@pytest.mark.parametrize('B,H,W,N', [(2, 7, 9, 8), (2, 5, 4, 8), (1, 66, 6, 8)])
def test_bilinear_comparator_rejects_wrong_gather_and_scatter(B, H, W, N):
    sizes, shape = pr.SIZES, (B, H, W, 8)
    q = pr.randn('cpu/sharp/q', (pr.rows(B, sizes), 9 * N))
    d = pr.randn('cpu/sharp/d', (B, H, W, N), torch.bfloat16)
    gref, gabs = pr.fact_gather(q, shape, sizes, N), pr.fact_gather(q.abs(), shape, sizes, N)
    sref, sabs = pr.fact_scatter(d, shape, sizes), pr.fact_scatter(d.abs(), shape, sizes)
    wrong = (('a border tap left unmasked', functools.partial(pr.tap_matrices, masked=False)),
             ('align_corners=True weights', functools.partial(pr.tap_matrices, interp=_align_corners)),
             ('source cell off by one', functools.partial(pr.tap_matrices, interp=_cell_off_by_one)))
    for dtype in BOTH:
        gb = pr.bilinear_bound(gref, gabs, dtype)
        assert pr.worst_ratio('gather: reference rounded to %s' % dtype, gref.to(dtype), gref, gb) <= 1
        floor = 1e3 if dtype == torch.float32 else 4
        for what, taps in wrong:
            assert pr.worst_ratio('gather: %s (%s)' % (what, dtype), pr.fact_gather(q, shape, sizes, N, taps), gref, gb) > floor
        assert pr.worst_ratio('gather: level 2 rows offset by one (%s)' % dtype, pr.fact_gather(_roll_level(q, B, sizes, 2), shape, sizes, N), gref, gb) > floor
    sb = pr.bilinear_bound(sref, sabs)
    assert pr.worst_ratio('scatter: reference rounded to fp32', sref.float(), sref, sb) <= 1
    for what, taps in wrong:
        assert pr.worst_ratio('scatter: %s' % what, pr.fact_scatter(d, shape, sizes, taps), sref, sb) > 1e3
    assert pr.worst_ratio('scatter: level 2 rows offset by one', _roll_level(sref, B, sizes, 2), sref, sb) > 1e3


def test_stage_bn_comparator_rejects_a_dropped_term_and_offset_rows():
    B, C, trains, no_gamma = pr.STAGE_BN_CASES['b5-c128']
    sizes = pr.SIZES
    x, dy, y, means, invs, gammas = pr.stage_bn_inputs('bn/b5-c128', B, C, sizes, trains, no_gamma)
    dx, dgs, dbs = pr.stage_bn_bwd(dy, y, x, B, sizes, means, invs, gammas, trains)
    ev, _, _ = pr.stage_bn_bwd(dy, y, x, B, sizes, means, invs, gammas, [False] * 4)          # the mean and projection terms dropped
    ungated, ug, ub = pr.stage_bn_bwd(dy, torch.ones_like(y), x, B, sizes, means, invs, gammas, trains)
    for l, sl in enumerate(pr.level_slices(B, sizes)):
        assert pr.worst_ratio('stage bn level %d: reference rounded to fp32' % l, dx[sl].float(), dx[sl], pr.max_bound(dx[sl])) <= 1
        if trains[l]:
            assert pr.worst_ratio('stage bn level %d: batch terms dropped' % l, ev[sl], dx[sl], pr.max_bound(dx[sl])) > 1e2
        assert pr.worst_ratio('stage bn level %d: ReLU gate dropped' % l, ungated[sl], dx[sl], pr.max_bound(dx[sl])) > 1e2
        assert pr.worst_ratio('stage bn level %d: dgamma without the gate' % l, ug[l], dgs[l], pr.max_bound(dgs[l])) > 1e2
        assert pr.worst_ratio('stage bn level %d: dbeta without the gate' % l, ub[l], dbs[l], pr.max_bound(dbs[l])) > 1e2
    # the last row of a level left out of the sums (a ragged last trip handled wrongly)
    sl = pr.level_slices(B, sizes)[3]
    short = (dy[sl][:-1].to(F64) * (y[sl][:-1] > 0)).sum(0)
    assert pr.worst_ratio('stage bn level 3: dbeta without the last row', short, dbs[3], pr.max_bound(dbs[3])) > 1e2


def test_one_row_train_level_has_a_zero_gradient_and_a_bound_of_its_own():
    """The B = 1 train case: the reference is exactly 0 on the one-row level, the fp32 three-term form evaluated as the kernel does stays inside stage_bn_dx_bound, and
    dividing the batch terms by a wrong count (2 instead of 1) is rejected."""
    B, C, trains, no_gamma = pr.STAGE_BN_CASES['b1-c32-one-row-level-train']
    assert trains[0] and B * pr.SIZES[0] ** 2 == 1
    x, dy, y, means, invs, gammas = pr.stage_bn_inputs('bn/b1-c32-one-row-level-train', B, C, pr.SIZES, trains, no_gamma)
    assert torch.equal(means[0], x[0])
    dx, dgs, dbs = pr.stage_bn_bwd(dy, y, x, B, pr.SIZES, means, invs, gammas, trains)
    sl = slice(0, 1)
    assert float(dx[sl].abs().max()) == 0 and float(dgs[0].abs().max()) == 0
    bound = pr.stage_bn_dx_bound(dx[sl], dy[sl], y[sl], invs[0], gammas[0], True)
    assert float((bound > 0).double().mean()) > 0.2
    g = dy[sl] * (y[sl] > 0)
    gi = gammas[0].double() * invs[0].double()
    form32 = gi.float() * g + (-gi * g.double()).float()                   # cA g + cC in fp32, coefficients rounded once from float64
    assert form32.dtype == torch.float32
    assert pr.worst_ratio('stage bn one-row train level: the fp32 three-term form', form32, dx[sl], bound) <= 0.75
    assert pr.worst_ratio('stage bn one-row train level: batch terms over count 2', gi * (g.double() - g.double() / 2), dx[sl], bound) > 1e5
